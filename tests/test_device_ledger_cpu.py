"""No GPU: the ledger of device resources (csrc/device_ledger.h, `tsd_debug_device_ledger`, `tsd.device_ledger()`).
(1) tests/cpp/device_ledger_main.cpp - a program of its own that includes nothing else of the project - is built with the host compiler
under AddressSanitizer and UBSan, and a second time under ThreadSanitizer, and run.  (2) No source of the library makes or releases a
device allocation, an event or a stream except through the dev_* wrappers of runtime.cpp, which are what feeds the ledger.  (3) Every
buffer a session allocates is in the one list its destroy releases.  (4) The exported entry answers without a device."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

import replay

CSRC = os.path.join(replay.ROOT, "stable-diffusion.mojo_amd", "csrc")
MAIN = os.path.join(replay.ROOT, "tests", "cpp", "device_ledger_main.cpp")
FIELDS = ["ALLOCS_LIVE", "BYTES_LIVE", "EVENTS_LIVE", "STREAMS_LIVE", "CTX_LIVE", "MODELS_LIVE", "SESSIONS_LIVE", "ALLOCS_TOTAL", "FREES_TOTAL",
          "FREES_UNKNOWN", "RELEASE_ERRORS"]


def _build(tmp_path, name, sanitize):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host g++")
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitize, "-pthread", "-I", CSRC, MAIN, "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run_clean(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "add up" in r.stdout


def test_ledger_counts_what_it_is_told_under_asan_and_ubsan(tmp_path):
    exe, b = _build(tmp_path, "device_ledger_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert b.returncode == 0, b.stderr
    _run_clean(exe)


def test_ledger_is_race_free_under_tsan(tmp_path):
    exe, b = _build(tmp_path, "device_ledger_tsan", ["-fsanitize=thread"])
    if b.returncode != 0:
        pytest.skip("this host compiler does not build or link -fsanitize=thread: " + b.stderr.strip()[-300:])
    _run_clean(exe)


# ---- the source check ---------------------------------------------------------------------------------------------------------------
RAW = re.compile(r"\bhip(Malloc\w*|Free\w*|HostMalloc|HostFree|EventCreate\w*|EventDestroy|StreamCreate\w*|StreamDestroy)\b")
WRAPPERS = ("dev_malloc", "dev_free", "dev_event_create", "dev_event_destroy", "dev_stream_create", "dev_stream_destroy")


def _code(text):
    """The text without comments and without the contents of string literals: what is left of a raw name is a use of it."""
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _without_wrapper_bodies(text):
    """runtime.cpp with the six wrapper definitions cut out; each must be there exactly once."""
    for w in WRAPPERS:
        text, n = re.subn(r"^hipError_t " + w + r"\([^)]*\) \{\n.*?^\}\n", "", text, flags=re.S | re.M)
        assert n == 1, f"runtime.cpp defines {w} {n} times"
    return text


def _raw_calls(path, text):
    return [f"{os.path.basename(path)}:{text.count(chr(10), 0, m.start()) + 1}: {m.group(0)}" for m in RAW.finditer(text)]


def _sources():
    files = sorted(f for ext in ("cpp", "h", "hip") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) > 30 and os.path.join(CSRC, "runtime.cpp") in files
    return files


def test_no_source_of_the_library_calls_the_runtime_for_a_resource_directly():
    found = []
    for f in _sources():
        text = _code(open(f).read())
        if os.path.basename(f) == "runtime.cpp":
            whole = _raw_calls(f, text)
            text = _without_wrapper_bodies(text)
            assert len(whole) - len(_raw_calls(f, text)) == len(WRAPPERS), "each wrapper makes exactly one call of the runtime"
        found += _raw_calls(f, text)
    assert not found, "raw device-resource calls outside the wrappers of runtime.cpp:\n  " + "\n  ".join(found)


def test_the_source_check_sees_a_raw_call_where_there_is_one():
    """The filter itself: code is seen, comments and string literals are not, and only the wrapper bodies are excused."""
    sample = ('// hipFree(p) in a comment\n/* hipMalloc(&p, n) */\nTSD_FAIL(E, "hipMalloc(%zu) failed");\n'
              "if (x) hipFree(x);\nHIP_TRY(hipEventCreateWithFlags(&e, 0));\nhipStreamCreate(&s); hipMallocAsync(&p, n, s);\n"
              "hipMemcpy(a, b, n, k); hipEventRecord(e, s); hipStreamSynchronize(s);\n")
    got = [c.split(": ")[1] for c in _raw_calls("x.cpp", _code(sample))]
    assert got == ["hipFree", "hipEventCreateWithFlags", "hipStreamCreate", "hipMallocAsync"]
    runtime = "hipError_t dev_free(void* p) {\n  const hipError_t e = hipFree(p);\n  return e;\n}\nvoid f() { hipFree(q); }\n"
    with pytest.raises(AssertionError):
        _without_wrapper_bodies(runtime)     # five wrappers are missing
    assert _raw_calls("runtime.cpp", re.sub(r"^hipError_t dev_free\([^)]*\) \{\n.*?^\}\n", "", runtime, flags=re.S | re.M)) == ["runtime.cpp:1: hipFree"]


def test_every_buffer_a_session_allocates_is_in_the_list_its_destroy_releases():
    """session.cpp: the targets of session_grow and of the state allocation are exactly the members session_release frees - the nine
    buffers tests/test_gpu_lifetime.py bounds a session's live allocations by."""
    src = _code(open(os.path.join(CSRC, "session.cpp")).read())
    owned = re.search(r"void\* const owned\[\] = \{([^}]*)\};", src).group(1)
    owned = [m.strip().replace("s->", "") for m in owned.split(",")]
    grown = set(re.findall(r"session_grow\(ctx, \(void\*\*\)&s->(\w+),", src)) | set(re.findall(r"dev_malloc\(\(void\*\*\)&s->(\w+),", src))
    assert len(owned) == len(set(owned)) == 9, owned
    assert grown == set(owned), (sorted(grown), sorted(owned))
    assert len(re.findall(r"\bdev_malloc\(", src)) == 2 and len(re.findall(r"\bdev_free\(", src)) == 2   # state + session_grow; grow + release
    destroy = src[src.index('int tsd_session_destroy('):]
    assert "session_release(s);" in destroy[:destroy.index("\n}\n")]


# ---- the exported entry ---------------------------------------------------------------------------------------------------------------
def test_ledger_entry_and_python_wrapper_without_a_device(tsd_mod):
    lib = tsd_mod._lib.lib()
    enum = replay.enum(open(replay.HDR).read(), "tsd_device_ledger_field")
    assert list(enum) == ["TSD_DL_" + f for f in FIELDS] + ["TSD_DL_COUNT"] and list(enum.values()) == list(range(len(FIELDS) + 1))
    n = len(FIELDS)
    out = (C.c_int64 * (n + 2))(*([-7] * (n + 2)))
    assert lib.tsd_debug_device_ledger(out, n + 2) == n           # never more than TSD_DL_COUNT fields
    assert list(out)[n:] == [-7, -7] and all(v >= 0 for v in list(out)[:n])
    two = (C.c_int64 * 3)(-7, -7, -7)
    assert lib.tsd_debug_device_ledger(two, 2) == n and two[2] == -7
    assert lib.tsd_debug_device_ledger(None, n) == tsd_mod._lib.TSD_E_ARG and b"tsd_debug_device_ledger" in lib.tsd_last_error()
    assert lib.tsd_debug_device_ledger(out, -1) == tsd_mod._lib.TSD_E_ARG
    d = tsd_mod.device_ledger()
    assert list(d) == FIELDS and d == dict(zip(FIELDS, list(out)[:n]))
    assert d["ALLOCS_LIVE"] == d["ALLOCS_TOTAL"] - d["FREES_TOTAL"]
    if lib.tsd_device_count() == 0:                               # nothing can have been allocated; a refused create counts no handle
        h = C.c_void_p()
        assert lib.tsd_ctx_create(0, C.byref(h)) == tsd_mod._lib.TSD_E_HIP
        assert tsd_mod.device_ledger() == dict.fromkeys(FIELDS, 0)
