"""GPU: the -DTSD_JITTER build (`make jitter`: a random wave-level delay at every point where waves meet - csrc/lds_dma.h lists them) held
to the SHIPPED library's bits over every replay sweep the fp64 tests run (tests/jitter_manifest.py: the forced tile configurations, the
split-K hand-offs, the V^T tail and the opt-in 256-row split of the GEMM kernel; the Sq / Sk edges of the five flash-attention instances
and the row-softmax kernels; the fused attention-block kernels at every T, pitched and batched; every GroupNorm statistics path and the
LayerNorm widths; k_small_linear in every instance; the LoRA merge), and over the product's graphs outside the headline shape.

The fp64 tests catch a kernel that is wrong every time.  A hazard between waves is wrong only when the waves drift apart: then the jitter
build gives other bits than the shipped schedule on the same operands.  Each test computes every case's digest once in this process with
the shipped library, starts ONE fresh child (TSD_LIB = the jitter library; never more than two processes on the GPU, no retry after a
failure) that runs every case REPEATS times, and asserts that the child reported exactly the manifest's names in order, the parent's status
for each, and the parent's digest in every repeat.

scripts/jitter_check.sh still runs the WHOLE suite on the jitter library by hand (there a test compares jittered output with the fp64 bound,
not with the shipped bits), and it is the only place the `diffusion_sd15` variant runs under jitter: that model's weight initialisation
alone takes longer than a test here may.

Wall time per test on an MI355X, parent and child together: gemm 6.4 s (980 cases), chain 2.8 s (31), norm 1.8 s
(140), attn 1.7 s (208), model graphs 1.1 s (5 cases, 4 repeats), lora 0.6 s (15), small linear 0.5 s (47), self-test 0.3 s.  Every case of
every family gave the shipped digest in all its repeats."""
import json
import os
import subprocess
import sys
import time

import pytest

import jitter_manifest as M

pytestmark = pytest.mark.gpu
REPEATS = 8
MODEL_REPEATS = 4
CHILD_TIMEOUT = 600


def _jitter_lib():
    if not os.path.exists(M.JITTER_LIB):
        pytest.skip(f"{M.JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    return M.JITTER_LIB


def _child(args, lib):
    """One fresh process on `lib`: its JSON lines.  A child that fails ends the test - nothing is started in its place."""
    env = dict(os.environ, TSD_LIB=lib)
    out = subprocess.run([sys.executable, M.__file__] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    return [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]


def _hold(tsd_mod, fam, part=None, repeats=REPEATS):
    jit = _jitter_lib()
    cases = M.select(fam, part)
    assert cases
    t0 = time.time()
    here = M.run_cases(tsd_mod, cases, 1)
    t1 = time.time()
    there = _child([fam, repeats] + ([f"{part[0]}/{part[1]}"] if part else []), jit)
    t2 = time.time()
    assert [r["name"] for r in there] == [c.name for c in cases], "the jitter child did not report exactly the manifest's cases, in order"
    bad = []
    for case, mine, theirs in zip(cases, here, there):
        what = f"{case.name} (forced cfg {case.extra})" if case.family == "gemm" else case.name
        if theirs["status"] != mine["status"]:
            bad.append(f"{what}: status {theirs['status']} under jitter, {mine['status']} shipped")
            continue
        assert len(theirs["digests"]) == repeats, f"{what}: {len(theirs['digests'])} of {repeats} repeats reported"
        diff = sum(dg != mine["digests"][0] for dg in theirs["digests"])
        if diff:
            bad.append(f"{what}: {diff} of {repeats} repeats differ from the shipped bits ({len(set(theirs['digests']))} distinct results)")
    refused = sum(r["status"] != 0 for r in here)
    print(f"\n[jitter] {fam}{'' if part is None else ' slice %d/%d' % part}: {len(cases)} cases ({refused} refused) x {repeats} repeats; "
          f"shipped {t1 - t0:.1f} s, jitter child {t2 - t1:.1f} s")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ under jitter:\n  " + "\n  ".join(bad[:40])


def test_gemm_sweeps_keep_the_shipped_bits_under_jitter(tsd_mod, gpu_ctx):
    """Every (case, forced configuration) pair of the tile sweep, the refused GNSTATS pairs with their status, the eight split-K cases, the
    V^T tail and the opt-in 256-row split (its own context): 980 cases, 6.4 s on an MI355X - well under the 20 s at which the family would be split
    into parametrised slices of its manifest (`jitter_manifest.py FAMILY REPEATS I/N` runs one; four of them took 1.7 - 2.0 s each)."""
    _hold(tsd_mod, "gemm")


def test_attention_sweeps_keep_the_shipped_bits_under_jitter(tsd_mod, gpu_ctx):
    """attn_ref.sweep() (five flash instances over the Sq / Sk edges and the score shapes) and the row-softmax sweep."""
    _hold(tsd_mod, "attn")


def test_chain_sweep_keeps_the_shipped_bits_under_jitter(tsd_mod, gpu_ctx):
    """chain_ref.NAMES: head and tail, every T, pitched, batched, 264 workgroups."""
    _hold(tsd_mod, "chain")


def test_norm_sweeps_keep_the_shipped_bits_under_jitter(tsd_mod, gpu_ctx):
    """Every GroupNorm statistics path of norm_ref.sweep() and the LayerNorm sweep over its eight widths."""
    _hold(tsd_mod, "norm")


def test_small_linear_sweep_keeps_the_shipped_bits_under_jitter(tsd_mod, gpu_ctx):
    """The SMALL_LINEAR family of elem_ref.sweep(): every NB instance, one and two K passes.  (The movement families have no wave hand-off.)"""
    _hold(tsd_mod, "elem")


def test_lora_merges_keep_the_shipped_bits_under_jitter(tsd_mod, gpu_ctx):
    """The three general-operand shapes and the twelve exact cases of test_gpu_lora.py through tsd_lora_merge_f32."""
    _hold(tsd_mod, "lora")


def test_model_graphs_outside_the_headline_shape_keep_the_shipped_bits_under_jitter(tsd_mod, gpu_ctx):
    """One denoise step of the default UNet with CFG at B = 2, L = 16 and without at B = 3, L = 24, Decoder.forward at a 16 x 16 latent,
    Encoder.forward at 128 px and CLIP at B = 2, 4 repeats each.  (B = 8, L = 64 is test_jitter_build_reproduces_the_shipped_bits; the
    diffusion_sd15 variant stays with scripts/jitter_check.sh: its weight initialisation alone exceeds a few seconds.)"""
    _hold(tsd_mod, "model", repeats=MODEL_REPEATS)


def test_the_jitter_build_makes_a_hazard_visible(tsd_mod, gpu_ctx):
    """tsd_debug_jitter_selftest: wave 0 reads an LDS word wave 1 writes, a jitter point in each, no barrier between.  64 launches on the
    jitter library must store at least 2 distinct words - a detector that shows nothing on a real hazard proves nothing with the tests
    above; the shipped library has no such kernel and says so.  Distinct words seen on an MI355X: 2 of the 2 possible (the word's initial 0 and the
    written value), in each of the three runs made."""
    jit = _jitter_lib()
    rc, msg = M.selftest(tsd_mod, 64)
    assert rc == tsd_mod._lib.TSD_E_ARG and "not supported in this build" in msg, (rc, msg)
    rec, = _child(["selftest", 64], jit)
    print(f"\n[jitter] self-test: {rec['distinct']} distinct words from 64 launches of the jitter build")
    assert rec["status"] == 0, rec
    assert rec["distinct"] >= 2, f"64 launches of the hazard kernel gave {rec['distinct']} distinct value(s): the jitter build perturbs nothing"
