"""No GPU: tests/norm_ref.py - the fp64 reference, the derived bound and the numpy emulation of csrc/kernels_norm.hip - is itself
tested.  The reference agrees with the oracle's norms on the op-level case shapes; its operand extents and its restatement of the
launch plan agree with tsd_debug_norm_run's sizing-only mode; the statistics share of the bound stays under its cap on every sweep
input; the emulation of the device arithmetic stays inside the bound on every sweep input, and every seeded defect is rejected."""
import numpy as np
import pytest

import norm_ref as N
import replay
from cases import CASES
from oracle import ops as O

SWEEP = N.sweep()
LN_SWEEP = N.ln_sweep()


def _size(tsd_mod, d, n=None):
    info = np.full(N.NI["COUNT"], -1, np.int64)
    rc, ext = replay.size("tsd_debug_norm_run", d, n, info)
    return rc, {s: int(ext[N.NO[s]]) for s in N.INPUTS + N.OUTPUTS}, {k: int(info[v]) for k, v in N.NI.items() if k != "COUNT"}


# ---- the reference against the oracle ---------------------------------------------------------------------------------------------
def _nhwc(x):
    c, h, w = x.shape
    return np.ascontiguousarray(x.reshape(c, h * w).T)[None].astype(np.float16).astype(np.float64)


def _chw(y, shape):
    return y.T.reshape(shape)


GN_CASES = [("groupnorm_320_32", 320, 32, 1e-5), ("groupnorm_960_32", 960, 32, 1e-5), ("groupnorm_320_320", 320, 320, 1e-5),
            ("groupnorm_128_16", 128, 16, 1e-5), ("groupnorm_eps1e-6", 640, 32, 1e-6), ("groupnorm_partial_channels", 64, 4, 1e-5),
            ("groupnorm_big_hw", 64, 32, 1e-5)]


@pytest.mark.parametrize("name,Cn,G,eps", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_reference_agrees_with_the_oracle_group_norm(name, Cn, G, eps):
    x = CASES[name].build()["x"][:Cn]
    x16 = x.astype(np.float16).astype(np.float32)
    xl = _nhwc(x16)
    d = N.gn_desc(xl.shape[1], Cn, G, B=1, eps=eps)
    ops = N.make_inputs(d, x=xl)
    ref, bd, _ = N.reference(d, ops, N.plan(d))
    want = O.group_norm(x16, G, Cn, eps).astype(np.float64)
    assert np.abs(_chw(ref, x16.shape) - want).max() <= 2e-5 * (1 + np.abs(want).max())   # the oracle works in fp32
    assert (bd < 2e-3 * (1 + np.abs(ref))).all()


GT_CASES = [("groupnorm_torch_320_32", 320, 32, 1e-5, True, False), ("groupnorm_torch_silu_1280", 1280, 32, 1e-5, True, True),
            ("groupnorm_torch_no_affine_big_hw", 64, 32, 1e-6, False, False)]


@pytest.mark.parametrize("name,Cn,G,eps,affine,silu", GT_CASES, ids=[c[0] for c in GT_CASES])
def test_reference_agrees_with_the_oracle_group_norm_torch(name, Cn, G, eps, affine, silu):
    i = CASES[name].build()
    x16 = i["x"].astype(np.float16).astype(np.float32)
    xl = _nhwc(x16)
    d = N.gn_desc(xl.shape[1], Cn, G, B=1, eps=eps, torch_rstd=1, has_w=int(affine), has_b=int(affine), silu=int(silu))
    ops = N.make_inputs(d, x=xl)
    if affine:
        ops["W"], ops["BIAS"] = i["w"].astype(np.float32), i["b"].astype(np.float32)
    ref, _, _ = N.reference(d, ops, N.plan(d))
    want = O.group_norm_torch(x16, G, eps, ops.get("W"), ops.get("BIAS")).astype(np.float64)
    want = O.silu(want) if silu else want
    assert np.abs(_chw(ref, x16.shape) - want).max() <= 2e-6 * (1 + np.abs(want).max())   # fp64 oracle, stored as fp32


LN_CASES = [("layernorm_320", 320, False, False), ("layernorm_1280", 1280, False, False), ("layernorm_torch_320", 320, True, True),
            ("layernorm_torch_640", 640, True, True), ("layernorm_torch_768", 768, True, True),
            ("layernorm_torch_1280_no_affine", 1280, True, False)]


@pytest.mark.parametrize("name,Cn,torch,affine", LN_CASES, ids=[c[0] for c in LN_CASES])
def test_reference_agrees_with_the_oracle_layer_norm(name, Cn, torch, affine):
    i = CASES[name].build()
    x16 = i["x"].astype(np.float16).astype(np.float32)
    d = N.ln_desc(x16.shape[0], Cn, torch_rstd=int(torch), has_w=int(affine), has_b=int(affine))
    ops = N.make_inputs(d, x=x16.astype(np.float64))
    if affine:
        ops["W"], ops["BIAS"] = i["w"].astype(np.float32), i["b"].astype(np.float32)
    ref, _, _ = N.reference(d, ops, None)
    want = (O.layer_norm_torch(x16, 1e-5, ops.get("W"), ops.get("BIAS")) if torch else O.layer_norm(x16)).astype(np.float64)
    assert np.abs(ref - want).max() <= 2e-5 * (1 + np.abs(want).max())


# ---- extents and plan against the entry's sizing-only mode ---------------------------------------------------------------------------
def test_extents_and_plan_agree_with_the_entry(tsd_mod):
    descs = [(n, d, e) for n, d, _, e in SWEEP] + [(n, d, None) for n, d in LN_SWEEP]
    for name, d, expect in descs:
        rc, ext, info = _size(tsd_mod, d)
        assert rc == 0, name
        assert ext == N.extents(d), f"{name}: the entry and tests/norm_ref.py size the operands differently"
        p = N.plan(d)
        assert {k: info[k] for k in p} == p, f"{name}: gn_plan {info} vs norm_ref.plan {p}"
        assert info["CHANGED"] == 0
        if expect is not None:
            assert {k: p[k] for k in expect} == expect, f"{name}: the case no longer reaches its path"


def test_unsizable_descriptors_are_refused(tsd_mod):
    good = N.gn_desc(64, 64, 32)
    for field, v in (("VERSION", 2), ("MODE", 7), ("B", 0), ("HW", 0), ("C", 0), ("GROUPS", 0), ("LD0", 56), ("LDY", 8), ("C0", 72),
                     ("SILU", 2), ("STATS", 3), ("HW", 1 << 40)):
        d = good.copy()
        d[N.ND[field]] = v
        assert _size(tsd_mod, d)[0] != 0, field
    d = N.gn_desc(64, 64, 32, stats=1, nslab=0)
    assert _size(tsd_mod, d)[0] != 0
    d = N.ln_desc(0, 64)
    assert _size(tsd_mod, d)[0] != 0
    assert replay.size("tsd_debug_norm_run", good, n=N.COUNT - 1)[0] != 0


# ---- the emulation inside the bound, the cap on the reference alone ------------------------------------------------------------------
@pytest.mark.parametrize("name,d,slab_rows,expect", SWEEP, ids=[s[0] for s in SWEEP])
def test_emulation_stays_inside_the_bound_and_the_cap_holds(name, d, slab_rows, expect):
    ops = N.make_inputs(d, seed=11, slab_rows=slab_rows)
    info = N.plan(d)
    if N.mode_of(d) != "GN_FINALIZE":
        assert N.well_conditioned(d, ops), "the sweep family promises |mean_g| <= 2 sigma_g"
    if N.mode_of(d) == "GROUPNORM":
        n, worst = N.cap_violations(d, ops, info)
        assert n == 0, f"statistics share of the bound above 2^-10 (|ref| + 1) at {n} elements (worst {worst:.3g} x cap)"
    fails, ratio = N.check(d, ops, N.emulate(d, ops, info), info)
    assert not fails, fails


def test_layernorm_emulation_stays_inside_the_bound_and_the_cap_holds():
    for name, d in LN_SWEEP:
        ops = N.make_inputs(d, seed=12)
        assert N.well_conditioned(d, ops), name
        n, worst = N.cap_violations(d, ops, None)
        assert n == 0, f"{name}: statistics share above the cap at {n} elements (worst {worst:.3g} x cap)"
        fails, _ = N.check(d, ops, N.emulate(d, ops, None), None)
        assert not fails, (name, fails)


def test_another_finalize_threshold_and_apply_multiplier_change_the_plan_only():
    d = dict((s[0], s[1]) for s in SWEEP)["fin_c320_g32_hw3072"]
    assert N.plan(d)["FINALIZE"] == 1 and N.plan(d, finalize_min=1 << 30)["FINALIZE"] == 0
    assert N.plan(d, apply_mult=4)["APPLY_PIXELS"] == 2 * N.plan(d)["APPLY_PIXELS"]


# ---- seeded defects -----------------------------------------------------------------------------------------------------------
def _edge(kind, **f):
    d = N.gn_desc(70, 128, 32, **f)
    return d, N.make_inputs(d, x=N.edge_inputs(kind))


def _mutations():
    by = dict((s[0], s) for s in SWEEP)
    ln = dict(LN_SWEEP)

    def sw(name):
        _, d, sr, _ = by[name]
        return d, N.make_inputs(d, seed=11, slab_rows=sr)
    return [
        ("one slab dropped from a 288-slab table", "drop_slab", lambda: sw("pre_ns288")),
        ("a prereduce chunk boundary off by one", "chunk_boundary", lambda: sw("pre_ns257")),
        ("sample b finished with sample 0's table", "sample0_table", lambda: sw("table_ns9")),
        ("two groups swapped", "swap_groups", lambda: sw("own_c320_g32_hw64")),
        ("comb consecutive fine groups from the wrong offset", "comb_offset", lambda: sw("comp_two_tables_comb3")),
        ("eps added to the variance instead of to sigma", "eps_in_var", lambda: _edge("small_sigma")),
        ("eps added to sigma instead of to the variance", "eps_on_sigma", lambda: _edge("small_sigma", torch_rstd=1)),
        ("second concat source read with the first one's pitch", "pitch_src1", lambda: sw("own_c960_two_sources")),
        ("the last HW % (PL * 4) pixels skipped", "skip_tail", lambda: sw("own_hw333_tail")),
        ("one LayerNorm row normalised with its neighbour's mean", "neighbour_mean",
         lambda: (ln["ln_c640_r53_w1b0_rstd1"], N.make_inputs(ln["ln_c640_r53_w1b0_rstd1"], seed=12))),
    ]


@pytest.mark.parametrize("what,mut,make", _mutations(), ids=[m[1] for m in _mutations()])
def test_seeded_defect_is_rejected(what, mut, make):
    d, ops = make()
    info = None if N.mode_of(d) == "LAYERNORM" else N.plan(d)
    fails, _ = N.check(d, ops, N.emulate(d, ops, info), info)
    assert not fails, f"the unmutated emulation must pass: {fails}"
    fails, ratio = N.check(d, ops, N.emulate(d, ops, info, mut=mut), info)
    assert fails and ratio > 2, f"{what}: not rejected (worst error {ratio:.3g} x bound)"


def test_both_eps_conventions_land_on_their_own_reference_at_small_sigma():
    """sigma ~ 1e-3: 1 / (sigma + eps) and 1 / sqrt(var + eps) differ by a factor of three - far more than the bound."""
    (d0, ops0), (d1, ops1) = _edge("small_sigma"), _edge("small_sigma", torch_rstd=1)
    r0, b0, _ = N.reference(d0, ops0, N.plan(d0))
    r1, b1, _ = N.reference(d1, ops1, N.plan(d1))
    assert np.median(np.abs(r0 - r1) / (b0 + b1)) > 100
