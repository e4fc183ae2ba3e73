"""GPU: the head-dimension-64 attention core, flash_attn_kernel<64, 1> (csrc/kernels_attn.hip), held to an fp64 reference element-wise
(tests/attn64_ref.py) through version-2 descriptors of tsd_debug_attn_run: B = 2 with batch-stride gaps, H = 5 and 20, pitches wider than
H * 64, the Sq / Sk edges of the loaders and of the tile loop (Sk = 577 and 641: a partial last tile behind the ninth, so the early look
of the optimistic pass runs), self-attention with the own-block reference on and off, the XCD map, attn_ref's score shapes (flat, equal
keys, rising, spike, self-peaked, very low, one-hot, subnormal tail, the overflow edge, a biased P rounding, two groups at 64 units), a
spike in key tile 9 of 10 (behind the early look: the final check must find it) and in tile 4 of 10 (in front of it), finite garbage in
the V^T pad columns, the refusals, and the jitter build's bits.  Every case asserts the status, kernel TSD_AK_64, that no guard or
pitch-gap element was written, the exact-repeat prediction, and every output element against the bound; it prints worst error / bound.

Worst error / bound seen on an MI355X: Sq sweep (1 ... 129, 77 keys, H = 5) 0.083 0.113 0.107 0.123 0.143 0.134
0.174; Sk sweep 0.000 (one key) 0.427 (Sk = 4, where the output rounding is most of the bound) 0.117 0.134 0.115 0.123 0.108 0.105 (63 ... 129)
0.055 0.053 (577, 641: the early look runs and finds nothing); H = 20 0.148 (129 x 65) 0.061 (33 x 641); self-peaked at 33 / 320 / 577 0.000
with the own-block reference on (no repeat) and off (320: 6 of 6, 577: 5 of 5 workgroups repeat); equal keys 0.012; rising 0.014, over a
partial last tile 0.045; spike in the last tile 0.029; scores near -300 0.000; one-hot 0.300; subnormal tail 0.178; overflow edge below /
across 16 units 0.055 / 0.046; biased P rounding 0.610 (no ones row: the 2^-11 sum w |v| term is used, as at d = 160); two score groups at 64
units 0.876 (the emulation gives the same figure: one fp16 rounding of Q at 64 units is most of the allowance); spike in tile 9 of 10 0.383
and in tile 4 of 10 0.043, 8 of 8 workgroups repeating in both, twice, same bits; XCD map 0.077, bitwise equal to the default block order;
V^T pad columns 0 and +-60000 at Sk = 7, 9, 77, 193 0.358 0.249 0.098 0.069, same bits; a sample alone and its row of B = 3 0.075, same bits.
No case fell into the "may" band of the exact-repeat prediction; no guard or pitch-gap element was written; the jitter build gave the shipped
digest in 8 of 8 repeats of all six cases.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attn64_ref as R
import attn_ref as A
import replay

pytestmark = pytest.mark.gpu
SWEEP = R.sweep()
NAMES = [s[0] for s in SWEEP]


@pytest.fixture(scope="module")
def ctx(gpu_ctx, tsd_mod):
    c = tsd_mod.Context(gpu_ctx.device)
    yield c
    c.close()


def run(ctx, d, ops):
    """(status, flat output, info {CHANGED, KERNEL, EXACT_WGS, DIAG, XCD_MAP})."""
    rc, outs, info = replay.run("tsd_debug_attn_run", ctx, d, ops, A.AO, A.INPUTS, ("O",), A.dtype_of, A.extents)
    return rc, outs["O"], {k: int(info[v]) for k, v in A.AI.items() if k != "COUNT"}


def verify(ctx, name, d, ops, ref=None, xcd=0):
    """Run d and hold it to the reference; returns (flat output, info, worst error / bound)."""
    rc, out, info = run(ctx, d, ops)
    assert rc == 0, f"{name}: status {rc}: {replay.lib().tsd_last_error().decode()}"
    p = R.plan(d, attn_xcd=xcd)
    assert p["KERNEL"] == A.AK["64"]
    assert {k: info[k] for k in p} == p, f"{name}: the launch took another path: {info}, expected {p}"
    assert info["CHANGED"] == 0, f"{name}: {info['CHANGED']} guard / pitch-gap elements written"
    replay.assert_gaps_hold_fill(out, A.o_index(d), f"{name}: O")
    pr = R.predict_repeat(d, ops)
    must, may = int((pr == 1).sum()), int((pr == 0).sum())
    fails, ratio = R.check(d, ops, out, ref=ref)
    print(f"[attn64] {name}: worst error / bound {ratio:.3f}  diag {info['DIAG']} xcd {info['XCD_MAP']} "
          f"exact repeats {info['EXACT_WGS']} (must {must}, may {may} more, of {pr.size})")
    assert must <= info["EXACT_WGS"] <= must + may, f"{name}: {info['EXACT_WGS']} workgroups repeated, prediction {pr.tolist()}"
    assert not fails, f"{name}: " + "; ".join(fails)
    return out, info, ratio


@pytest.mark.parametrize("name", NAMES)
def test_d64_kernel_matches_the_fp64_reference(ctx, name):
    d, kind, ops, ref = R.case(name)
    if kind != "onehot":
        assert R.well_conditioned(d, ops)
    verify(ctx, name, d, ops, ref)


def test_spike_behind_and_in_front_of_the_early_look_repeat_exactly_as_predicted(ctx):
    """Ten key tiles: the only early look comes after tile 8.  A spike in tile 9 is the final check's to find, one in tile 4 the early
    look's; either way every workgroup repeats, exactly as predict_repeat says (no 'may' band), and the bits of the two runs of each are
    equal (the look changes when a pass ends, never a result)."""
    for name in ("spike_t9of10", "spike_t4of10"):
        d, _, ops, ref = R.case(name)
        pr = R.predict_repeat(d, ops)
        assert (pr == 1).all(), f"{name}: the prediction is not 'must' everywhere: {pr.tolist()}"
        y0, i0, _ = verify(ctx, name, d, ops, ref)
        y1, i1, _ = verify(ctx, name + "/again", d, ops, ref)
        assert i0["EXACT_WGS"] == i1["EXACT_WGS"] == pr.size
        assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16))


def test_xcd_map_gives_the_same_bits(ctx, gpu_ctx, tsd_mod, monkeypatch):
    c = replay.ctx_with(tsd_mod, gpu_ctx, monkeypatch, "TSD_ATTN_XCD", 1)
    try:
        d = R.attn_desc(2, 8, 256, 512)
        ops = R.make_inputs(d, "flat", seed=13)
        ref = R.reference(d, ops)
        y0, i0, _ = verify(ctx, "xcd0", d, ops, ref)
        y1, i1, _ = verify(c, "xcd1", d, ops, ref, xcd=1)
        assert i0["XCD_MAP"] == 0 and i1["XCD_MAP"] == 1
        assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16)), "the XCD map changed a bit of the output"
    finally:
        c.close()


PADS = R.pad_sweep()


@pytest.mark.parametrize("name,d", PADS, ids=[p[0] for p in PADS])
def test_finite_pad_columns_of_vt_do_not_change_a_bit(ctx, name, d):
    z = R.make_inputs(d, "flat", seed=7, pad=0.0)
    f = R.make_inputs(d, "flat", seed=7, pad=A.pad_fill(d))
    assert A.skv_of(d) > A.F(d, "SK") and not np.array_equal(z["VT"].view(np.uint16), f["VT"].view(np.uint16))
    ref = R.reference(d, z)
    y0, _, _ = verify(ctx, name + "/zero", d, z, ref)
    y1, _, _ = verify(ctx, name + "/60000", d, f, ref)
    assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16)), f"{name}: the V^T pad columns reached the output"


def test_run_to_run_and_batch_invariance_are_bitwise(ctx):
    """A sample alone gives the bits of its row of B = 3 (one kernel at every shape; nothing keys on the batch)."""
    d3 = R.attn_desc(3, 5, 129, 321)
    ops3 = R.make_inputs(d3, "flat", seed=21)
    y3, _, _ = verify(ctx, "b3", d3, ops3)
    y3b, _, _ = verify(ctx, "b3/again", d3, ops3)
    assert np.array_equal(y3.view(np.uint16), y3b.view(np.uint16))
    q, k, v, _ = A.unpack_inputs(d3, ops3)
    d1 = R.attn_desc(1, 5, 129, 321)
    for b in range(3):
        ops1 = A.pack(d1, q[b:b + 1], k[b:b + 1], v[b:b + 1])
        y1, _, _ = verify(ctx, f"b1/{b}", d1, ops1)
        assert np.array_equal(A.unpack_output(d1, y1)[0].view(np.uint16), A.unpack_output(d3, y3)[b].view(np.uint16)), b


@pytest.mark.parametrize("name,d", [("head_dim_48_v2", R.attn_desc(1, 2, 8, 16, hd=48)), ("head_dim_64_v1", R.attn_desc(1, 1, 8, 16, version=1)),
                                    ("head_dim_64_v1_h5", R.attn_desc(1, 5, 33, 77, version=1))], ids=lambda x: x if isinstance(x, str) else "")
def test_refused_launches_leave_the_output_untouched(ctx, name, d):
    r = np.random.default_rng(3)
    ext = A.extents(d)
    ops = {s: r.standard_normal(ext[s]).astype(np.float16) for s in ("Q", "K", "VT")}
    rc, out, info = run(ctx, d, ops)
    assert rc != 0, f"{name} was not refused"
    assert all(v == 0 for v in info.values()), info
    replay.assert_untouched({"O": out}, name)


# ---- the jitter build --------------------------------------------------------------------------------------------------------------
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
JITTER_REPEATS = 8


def jitter_cases(c, repeats):
    """[(name, [digest per repeat])] of attn64_ref.JITTER_CASES on context c (of whatever library TSD_LIB names)."""
    out = []
    for name in R.JITTER_CASES:
        d, _, ops, _ = R.case(name)
        digs = []
        for _ in range(repeats):
            rc, y, info = run(c, d, ops)
            assert rc == 0 and info["KERNEL"] == A.AK["64"], (name, rc, info)
            digs.append(hashlib.sha256(y.view(np.uint16).tobytes()).hexdigest()[:16])
        out.append((name, digs))
    return out


def test_jitter_build_reproduces_the_shipped_bits(ctx):
    """A fresh child process on lib/libtsd_jitter.so (random wave-level delays at every tile step and barrier): six d = 64 cases, 8
    repeats each, every digest equal to the shipped library's digest in this process."""
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    here = jitter_cases(ctx, 1)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [r["name"] for r in there] == [n for n, _ in here]
    for (name, mine), theirs in zip(here, there):
        assert len(theirs["digests"]) == JITTER_REPEATS
        assert all(dg == mine[0] for dg in theirs["digests"]), f"{name}: the jitter build gave {len(set(theirs['digests']))} result(s), not the shipped bits"


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "stable-diffusion.mojo_amd")]
    import tsd
    tsd.set_strict(True)
    _c = tsd.Context(0)
    for _name, _digests in jitter_cases(_c, int(sys.argv[2])):
        print(json.dumps({"name": _name, "digests": _digests}), flush=True)
    _c.close()
