"""No GPU: the scan behind the "guard / pitch-gap elements the launch changed" count of the replay entries (csrc/replay_scan.h) is
shown to count a write where there is one.  tests/cpp/replay_scan_main.cpp - a program of its own that includes nothing else of the
project - is built with the host compiler under AddressSanitizer and UBSan and run."""
import os
import shutil
import subprocess

import pytest

import replay

CSRC = os.path.join(replay.ROOT, "stable-diffusion.mojo_amd", "csrc")
MAIN = os.path.join(replay.ROOT, "tests", "cpp", "replay_scan_main.cpp")


def test_scan_counts_every_write_outside_the_logical_elements(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host g++")
    exe = str(tmp_path / "replay_scan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, MAIN, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "counted once" in r.stdout
