"""No GPU: tests/attn_ref.py - the fp64 reference, the derived bound, the exact-repeat prediction and the numpy emulation of
csrc/kernels_attn.hip / kernels_attn8.hip and of the row-softmax kernels - is itself tested.  The reference agrees with the oracle's
attention; the operand extents and the dispatcher's choice agree with tsd_debug_attn_run's sizing-only mode (production shapes and one
shape just below each threshold pinned); the emulation stays inside the bound on every sweep input and takes the exact repeat where
the prediction says it must; every seeded defect that can change an output is rejected on a sweep input the GPU test runs too."""
import numpy as np
import pytest

import attn_ref as A
import replay
from oracle import ops as O

SWEEP = A.sweep()
NAMES = [s[0] for s in SWEEP]


def _size(tsd_mod, d, n=None):
    info = np.full(A.AI["COUNT"], -1, np.int64)
    rc, ext = replay.size("tsd_debug_attn_run", d, n, info)
    return rc, {s: int(ext[A.AO[s]]) for s in A.INPUTS + ("O",)}, {k: int(info[v]) for k, v in A.AI.items() if k != "COUNT"}


# ---- the reference against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,hd,Sq,Sk", [(8, 40, 64, 77), (2, 80, 33, 129), (1, 160, 16, 16)])
def test_reference_agrees_with_the_oracle_attention(H, hd, Sq, Sk):
    d = A.attn_desc(1, H, hd, Sq, Sk)
    ops = A.make_inputs(d, "flat", seed=3)
    q, k, v, _ = (x.astype(np.float32) for x in A.unpack_inputs(d, ops))
    tok = lambda x: np.ascontiguousarray(x[0].transpose(1, 0, 2).reshape(x.shape[2], H * hd))
    want = O.attention_core(tok(q), tok(k), tok(v), H).astype(np.float64)
    ref, bd = A.reference(d, ops)
    assert np.abs(tok(ref[:, :, :, :]) - want).max() <= 2e-5 * (1 + np.abs(want).max())   # the oracle works in fp32
    assert (bd < 1e-2 * (1 + np.abs(ref))).all()      # (sanity: the bound is small against the signal on plain inputs)


# ---- sizing and the dispatcher ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,kind", SWEEP[::7], ids=NAMES[::7])
def test_sizing_call_agrees_with_attn_ref(tsd_mod, name, d, kind):
    rc, ext, info = _size(tsd_mod, d)
    assert rc == 0, tsd_mod._lib.lib().tsd_last_error().decode()
    assert ext == A.extents(d)
    p = A.plan(d)
    assert {k: info[k] for k in p} == p
    assert info["CHANGED"] == 0 and info["EXACT_WGS"] == 0


def test_dispatcher_choice_is_pinned_from_the_sizing_call(tsd_mod):
    """The production shapes and one shape just below each threshold (Sk = 511; ceil(Sq / 512) H = 63, which falls to the 4-wave
    64-query kernel; ceil(Sq / 256) H = 63, which falls to 32 queries per wave)."""
    want = {
        (2, 8, 40, 4096, 4096): "40_8W", (2, 8, 40, 4096, 77): "40_1", (2, 8, 80, 1024, 1024): "80", (2, 8, 160, 256, 256): "160",
        (1, 8, 40, 4096, 511): "40_1", (1, 8, 40, 4096, 512): "40_8W",
        (1, 9, 40, 3584, 512): "40_2",       # ceil(3584 / 512) * 9 = 63 < 64, ceil(3584 / 256) * 9 = 126
        (1, 8, 40, 3585, 512): "40_8W",      # ceil(3585 / 512) * 8 = 64
        (1, 9, 40, 1792, 512): "40_1",       # ceil(1792 / 256) * 9 = 63 < 64
        (1, 8, 40, 1793, 512): "40_2",       # ceil(1793 / 256) * 8 = 64, ceil(1793 / 512) * 8 = 32
    }
    for (B, H, hd, Sq, Sk), kern in want.items():
        d = A.attn_desc(B, H, hd, Sq, Sk, dense=True)
        rc, ext, info = _size(tsd_mod, d)
        assert rc == 0 and info["KERNEL"] == A.AK[kern] == A.plan(d)["KERNEL"], ((B, H, hd, Sq, Sk), info, kern)
        assert info["DIAG"] == (1 if Sq == Sk else 0) and info["XCD_MAP"] == 0
    for mode, kern in ((1, "40_1"), (2, "40_2"), (3, "40_8W")):      # a forced mode wins at any shape
        assert _size(tsd_mod, A.attn_desc(1, 2, 40, 33, 77, kernel=mode))[2]["KERNEL"] == A.AK[kern]
    assert A.plan(A.attn_desc(2, 8, 40, 256, 512), attn_xcd=1)["XCD_MAP"] == 1


def test_descriptors_that_cannot_be_sized_are_refused(tsd_mod):
    good = A.attn_desc(2, 2, 40, 33, 77)
    assert _size(tsd_mod, good)[0] == 0
    assert _size(tsd_mod, good, n=A.COUNT - 1)[0] != 0
    for f, v in (("VERSION", 7), ("MODE", 5), ("B", 0), ("H", 0), ("LDQ", 72), ("LDVT", 76), ("SQB", 10), ("KERNEL", 4), ("DIAG", 2),
                 ("SQ", -1)):
        bad = good.copy()
        bad[A.AD[f]] = v
        assert _size(tsd_mod, bad)[0] != 0, f
    sm = A.softmax_desc(3, 77, ld=88, dtype=1, causal=77, zero_to=80)
    assert _size(tsd_mod, sm)[0] == 0 and _size(tsd_mod, sm)[1]["X"] == 2 * 88 + 80
    for f, v in (("LD", 76), ("ZERO_TO", 89), ("DTYPE", 2), ("ROWS", 0)):
        bad = sm.copy()
        bad[A.AD[f]] = v
        assert _size(tsd_mod, bad)[0] != 0, f
    assert _size(tsd_mod, A.softmax_desc(3, 77, ld=88, dtype=0))[0] != 0      # the fp32 launch is dense
    # the shapes the launcher itself refuses are sized: head dimension, misaligned pitches, empty sequences (as one row)
    for d in (A.attn_desc(1, 2, 48, 8, 8), A.attn_desc(1, 2, 40, 8, 8, ldq=84), A.attn_desc(1, 2, 40, 0, 8), A.attn_desc(1, 2, 40, 8, 0)):
        rc, ext, info = _size(tsd_mod, d)
        assert rc == 0 and ext == A.extents(d) and info["KERNEL"] in (0, A.AK["40_1"])


# ---- the emulation inside the bound, the prediction ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_inside_the_bound(name):
    d, kind, ops, ref = A.case(name)
    if kind != "onehot":
        assert A.well_conditioned(d, ops)
    y, repeats = A.emulate(d, ops)
    fails, ratio = A.check(d, ops, y, ref=ref)
    assert not fails and ratio <= 1.0, f"{name}: {fails}"
    pr = A.predict_repeat(d, ops)
    assert (pr == 1).sum() <= repeats <= (pr >= 0).sum(), f"{name}: {repeats} repeats, prediction {pr.tolist()}"
    assert np.array_equal(np.isnan(y), np.isnan(A.pack_output(d, np.zeros(ref[0].shape))))       # the gaps keep the fill


def test_prediction_covers_must_must_not_and_the_edge():
    lo, hi = A.case("40_1/edge_lo"), A.case("40_1/edge_hi")
    assert (A.predict_repeat(lo[0], lo[2]) == -1).all() and (A.predict_repeat(hi[0], hi[2]) == 1).all()
    for name, want in (("40_2/self320/diag1", -1), ("40_2/self320/diag0", 1), ("40_8w/rising", 1), ("160/spike", 1), ("80/subtail", -1)):
        d, _, ops, _ = A.case(name)
        assert (A.predict_repeat(d, ops) == want).all(), name


# ---- seeded defects ----------------------------------------------------------------------------------------------------------------
DEFECT_CASES = {   # every one a case tests/test_gpu_attn_ref.py runs on the device
    "drop_last_key": ("40_1/sk77", "40_8w/sk193", "160/sk65"),
    "admit_masked_key": ("40_1/sk77", "80/sk9"),
    "scale_sqrt48": ("40_1/sq129", "40_2/sk320", "40_8w/sk1152"),
    "v_swap_bits23": ("40_1/sk64", "40_8w/sk576", "160/sk8"),
    "head_offset_b": ("40_1/sq33", "40_2/sq257", "80/sk129"),
    "no_alpha": ("40_1/rising", "40_2/edge_hi", "40_8w/rising", "160/rising"),
    "flush_subnormal_p": tuple(f"{kn}/subtail" for kn, _, _ in A.KERNELS),
    "sum_unrounded_p": ("40_1/pbias", "40_2/pbias", "40_8w/pbias"),
    "q_double_round": ("40_1/qdouble", "80/qdouble"),
    "pad_weight_2m24": ("40_1/pad_sk7", "40_8w/pad_sk77", "160/pad_sk193"),
}


@pytest.mark.parametrize("mut", sorted(DEFECT_CASES))
def test_seeded_defect_is_rejected(mut):
    for name in DEFECT_CASES[mut]:
        if "/pad_" in name:
            d = dict(A.pad_sweep())[name]
            ops = A.make_inputs(d, "flat", seed=7, pad=A.pad_fill(d))
            ref = A.reference(d, ops)
        else:
            d, _, ops, ref = A.case(name)
        good, _ = A.emulate(d, ops)
        assert not A.check(d, ops, good, ref=ref)[0], f"{name}: the unmodified emulation fails"
        bad, _ = A.emulate(d, ops, mut=mut)
        fails, ratio = A.check(d, ops, bad, ref=ref)
        assert fails and ratio > 1.0, f"{mut} passes on {name} (worst error / bound {ratio:.3f})"


def test_a_zero_row_in_place_of_the_row_clamp_cannot_change_an_output():
    """The loaders clamp qrow >= Sq to row Sq - 1.  The clamped rows are never stored; they can reach an output only through what a
    wave or a workgroup decides together - the exact repeat, and the reference moves of the repeat.  A copy of row Sq - 1 overflows
    and moves exactly when row Sq - 1 does, and a zero row (every score 0, its own reference 0 + HEADROOM) never does either, so
    loading zeros instead changes no decision and no output bit: this defect is not observable, by construction, and the emulation
    says the same on shapes with clamped rows in both passes.  (What the clamp protects against is the read itself: a row past the
    operand; the NaN guard bands and the pitch-gap NaN of tests/test_gpu_attn_ref.py would show that as a spurious exact repeat.)"""
    for name in ("40_1/sq129", "40_2/sq257", "40_8w/sq513", "40_2/self577/diag0", "40_8w/rising", "160/rising", "80/spike"):
        d, _, ops, _ = A.case(name)
        assert A.F(d, "SQ") % A.WG_ROWS[A.plan(d)["KERNEL"]]
        y0, r0 = A.emulate(d, ops)
        y1, r1 = A.emulate(d, ops, mut="clamp_zero_row")
        assert r0 == r1 and np.array_equal(y0.view(np.uint16), y1.view(np.uint16)), name


# ---- row softmax ---------------------------------------------------------------------------------------------------------------------
SM_SWEEP = A.softmax_sweep()


@pytest.mark.parametrize("name,d", SM_SWEEP, ids=[s[0] for s in SM_SWEEP])
def test_softmax_emulation_stays_inside_the_bound_and_defects_do_not(tsd_mod, name, d):
    rc, ext, _ = _size(tsd_mod, d)
    assert rc == 0 and ext == A.extents(d)
    x = A.softmax_inputs(d, seed=5)
    ref = A.softmax_reference(d, x)
    fails, ratio = A.softmax_check(d, x, A.softmax_emulate(d, x), ref=ref)
    assert not fails and ratio <= 1.0, fails
    rows = A._softmax_rows_of(d, x, A.F(d, "COLS")).astype(np.float64)
    kept = A.softmax_kept(d)
    want = np.stack([np.pad(O.softmax_lastdim(r[None, :n].astype(np.float32))[0], (0, len(r) - n)) for r, n in zip(rows, kept)])
    assert np.abs(ref[0][:, :len(rows[0])] - want).max() <= 1e-6
    muts = ["exp2_without_log2e", "sum_skips_last_chunk"] + (["causal_off_by_one"] if A.F(d, "CAUSAL") else [])
    for mut in muts:
        if mut == "sum_skips_last_chunk" and (kept % 256 == 0).all():
            continue
        assert A.softmax_check(d, x, A.softmax_emulate(d, x, mut=mut), ref=ref)[0], f"{mut} passes on {name}"
