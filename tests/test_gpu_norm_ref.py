"""GPU: the GroupNorm / LayerNorm kernels (csrc/kernels_norm.hip) held to an fp64 reference element-wise (tests/norm_ref.py) through
tsd_debug_norm_run - every statistics path launch_groupnorm chooses (own pass, producer table finished in the apply blocks or by
the finalize launch, prereduce, composite), the statistics-only entries, two-source loads, pitches, B > 1, widths above 2048
channels, the affine / SiLU variants, both LayerNorm kernels around their rows per block, and the documented refusals.  Every case
asserts the path the launch reports, that no guard or pitch-gap element was written, and every output element against the bound.

Worst error / bound seen per path on an MI355X: own pass 0.99, own pass + finalize 0.99, table 1.00,
prereduce 1.00, composite 1.00 (an fp16 output half an ulp from the reference sits at the bound by construction), statistics-only
0.02, LayerNorm 0.99."""
import ctypes as C

import numpy as np
import pytest

import norm_ref as N
import replay

pytestmark = pytest.mark.gpu
_i64p = C.POINTER(C.c_int64)
SEED = 1234
SWEEP = N.sweep()
BY_NAME = {s[0]: s for s in SWEEP}


@pytest.fixture(scope="module")
def ctx(gpu_ctx, tsd_mod):
    c = tsd_mod.Context(gpu_ctx.device)
    yield c
    c.close()


def run(ctx, d, ops):
    """(status, outputs {Y, STATS}, info {CHANGED, NSLAB, OWN_PASS, ...})."""
    rc, outs, info = replay.run("tsd_debug_norm_run", ctx, d, ops, N.NO, N.INPUTS, N.OUTPUTS, N.dtype_of, N.extents)
    return rc, outs, {k: int(info[v]) for k, v in N.NI.items() if k != "COUNT"}


def verify(ctx, name, d, ops, expect=None):
    """Run d and hold it to the reference; returns (output, info, worst error / bound)."""
    rc, outs, info = run(ctx, d, ops)
    assert rc == 0, f"{name}: status {rc}: {replay.lib().tsd_last_error().decode()}"
    if expect is not None:
        assert {k: info[k] for k in expect} == expect, f"{name}: the launch took another path: {info}"
    assert info["CHANGED"] == 0, f"{name}: {info['CHANGED']} guard / pitch-gap elements written"
    out = outs["Y"] if "Y" in outs else outs["STATS"]
    fails, ratio = N.check(d, ops, out, info)
    print(f"[norm] {name}: worst error / bound {ratio:.3f}  path {info}")
    assert not fails, f"{name}: " + "; ".join(fails)
    if "Y" in outs:  # the pitch gaps of y still hold the fill
        rows = N.F(d, "ROWS") if N.mode_of(d) == "LAYERNORM" else N.F(d, "B") * N.F(d, "HW")
        replay.assert_gaps_hold_fill(out, np.arange(rows)[:, None] * N.F(d, "LDY") + np.arange(N.F(d, "C"))[None, :], f"{name}: y")
    return out, info, ratio


# ---- GroupNorm: every statistics path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,slab_rows,expect", SWEEP, ids=[s[0] for s in SWEEP])
def test_groupnorm_path_matches_the_fp64_reference(ctx, name, d, slab_rows, expect):
    ops = N.make_inputs(d, seed=11, slab_rows=slab_rows)
    if N.mode_of(d) != "GN_FINALIZE":
        assert N.well_conditioned(d, ops)
    verify(ctx, name, d, ops, expect)
    if name.startswith("table_"):  # the same x through the launch's own statistics pass: held to the same bound function
        own = d.copy()
        own[N.ND["STATS"]] = 0
        own[N.ND["NSLAB"]] = 0
        _, info, _ = verify(ctx, name + "/own", own, {k: v for k, v in ops.items() if k != "PART0"})
        assert info["OWN_PASS"] == 1 and info["PREREDUCE"] == 0 and info["COMPOSITE"] == 0


FINALIZE_CASES = ("fin_c320_g320_hw576", "fin_c320_g32_hw3072", "table_ns128", "table_ns200", "pre_ns288", "comp_two_tables_finalize")


def test_finalize_launch_and_in_block_finish_give_the_same_bits(ctx, gpu_ctx, tsd_mod, monkeypatch):
    """k_gn_finalize and the apply blocks' own finish add the same doubles in the same order: with the threshold out of reach the
    launch disappears and not one bit of the output moves."""
    c = replay.ctx_with(tsd_mod, gpu_ctx, monkeypatch, "TSD_GN_FINALIZE_MIN", 1 << 30)
    try:
        for name in FINALIZE_CASES:
            _, d, sr, expect = BY_NAME[name]
            ops = N.make_inputs(d, seed=11, slab_rows=sr)
            y0, i0, _ = verify(ctx, name, d, ops, expect)
            y1, i1, _ = verify(c, name + "/in-block", d, ops, dict(expect, FINALIZE=0))
            assert i0["FINALIZE"] == 1 and i1["FINALIZE"] == 0
            assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16)), f"{name}: the finalize launch and the in-block finish differ"
    finally:
        c.close()


@pytest.mark.parametrize("mult", (1, 4))
def test_apply_multiplier_does_not_change_a_bit(ctx, gpu_ctx, tsd_mod, monkeypatch, mult):
    c = replay.ctx_with(tsd_mod, gpu_ctx, monkeypatch, "TSD_GN_APPLY_MULT", mult)
    try:
        for name in ("own_c64_hw1920", "own_c96_pitches", "own_c960_two_sources", "own_c2560_two_chunks", "own_hw333_tail", "table_ns9",
                     "fin_c320_g32_hw3072", "affine_w1b1_rstd1_silu1"):
            _, d, sr, expect = BY_NAME[name]
            ops = N.make_inputs(d, seed=11, slab_rows=sr)
            y0, i0, _ = verify(ctx, name, d, ops, expect)
            y1, i1, _ = verify(c, f"{name}/mult{mult}", d, ops, expect)
            assert i1["APPLY_PIXELS"] * 2 == i0["APPLY_PIXELS"] * mult
            assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16)), f"{name}: apply blocks of {i1['APPLY_PIXELS']} pixels differ"
    finally:
        c.close()


# ---- conditioning edges (outside the cap of the main sweep) ---------------------------------------------------------------------------
def _edge(kind, **f):
    d = N.gn_desc(70, 128, 32, **f)
    return d, N.make_inputs(d, x=N.edge_inputs(kind))


def test_both_eps_conventions_land_on_their_own_reference_at_small_sigma(ctx):
    refs = []
    for tr in (0, 1):
        d, ops = _edge("small_sigma", torch_rstd=tr)
        verify(ctx, f"small_sigma_rstd{tr}", d, ops)
        refs.append(N.reference(d, ops, N.plan(d)))
    assert np.median(np.abs(refs[0][0] - refs[1][0]) / (refs[0][1] + refs[1][1])) > 100   # the conventions are far apart here


def test_cancellation_stays_inside_the_derived_bound(ctx):
    for silu in (0, 1):
        d, ops = _edge("cancellation", silu=silu)
        verify(ctx, f"cancellation_silu{silu}", d, ops)


def test_constant_group_is_finite_and_zero_group_is_exact(ctx):
    for silu in (0, 1):
        for tr in (0, 1):
            d, ops = _edge("constant", silu=silu, torch_rstd=tr)
            rc, outs, info = run(ctx, d, ops)
            assert rc == 0 and info["CHANGED"] == 0
            y = N.unpack(outs["Y"], 3 * 70, 128, 128).astype(np.float64)
            assert np.isfinite(y).all(), "a constant group gave a non-finite output"
            d, ops = _edge("zero", silu=silu, torch_rstd=tr)
            y, _, _ = verify(ctx, f"zero_group_silu{silu}_rstd{tr}", d, ops)
            z = N.unpack(y, 3 * 70, 128, 128).reshape(3, 70, 32, 4)[:, :, 2]
            assert (z.view(np.uint16) & 0x7FFF == 0).all(), "an all-zero group is not exactly zero"


# ---- SiLU: the hardware exp2 / rcp term ------------------------------------------------------------------------------------------
def test_silu_only_run_measures_the_hardware_term(ctx):
    """A table that says mean 0, variance 1 (eps = 0, gamma = 1) turns the apply line into y = fp16(silu(x)): every fp16 value in
    (-20, 20) goes through it.  An output on the wrong side of a rounding midpoint proves an fp32 error of at least the reference's
    distance to that midpoint; the largest such distance, relative to the result, is the measured term norm_ref.SILU_HW allows 4x."""
    half = np.arange(0x4D00, dtype=np.uint16)                       # +0 ... just below 20.0
    x = np.concatenate([half, half | 0x8000]).view(np.float16).astype(np.float64).reshape(1, 616, 64)
    d = N.gn_desc(616, 64, 32, B=1, stats=1, nslab=1, eps=0.0, silu=1)
    ops = N.make_inputs(d, x=x, slab_rows=616)
    ops["PART0"] = np.tile(np.array([0.0, 2 * 616.0], np.float32), 32)
    y, info, _ = verify(ctx, "silu_only", d, ops, dict(OWN_PASS=0, NSLAB=1, FINALIZE=0))
    ref = N.silu64(x.reshape(616, 64))
    got = N.unpack(y, 616, 64, 64)
    best = ref.astype(np.float16)
    off = (got != best) & (np.abs(ref) >= 2.0 ** -14)
    mid = (got.astype(np.float64) + best.astype(np.float64)) / 2
    dev = np.where(off, np.abs(ref - mid) / np.maximum(np.abs(ref), 1e-300), 0.0)
    print(f"[norm] silu_only: {int(off.sum())} of {off.size} outputs are not the correctly rounded result; largest proven fp32 "
          f"deviation {dev.max() / N.U32:.3f} u at x = {x.reshape(-1)[int(np.argmax(dev))]!r} (allowance {N.SILU_HW / N.U32:.1f} u)")
    assert dev.max() <= N.SILU_HW


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", (320, 640, 1280, 8, 64, 768, 1024, 2048))
def test_layernorm_matches_the_fp64_reference(ctx, width):
    cases = [(n, d) for n, d in N.ln_sweep() if N.F(d, "C") == width]
    rpb = N.ln_rows_per_block(width)
    assert {N.F(d, "ROWS") for _, d in cases} == {1, rpb - 1, rpb, rpb + 1, 3 * rpb + 5}
    assert len({(N.F(d, "HAS_W"), N.F(d, "HAS_B"), N.F(d, "TORCH_RSTD")) for _, d in cases}) == 8
    worst = 0.0
    for name, d in cases:
        ops = N.make_inputs(d, seed=12)
        _, info, ratio = verify(ctx, name, d, ops)
        worst = max(worst, ratio)
    print(f"[norm] layernorm C = {width}: worst error / bound {worst:.3f} over {len(cases)} launches")


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _refusals():
    return [
        ("gn_c_not_multiple_of_8", N.gn_desc(16, 12, 4)),
        ("gn_c_not_multiple_of_groups", N.gn_desc(16, 64, 48)),
        ("gn_c_above_4096", N.gn_desc(4, 4104, 8)),
        ("gn_c0_not_multiple_of_8", N.gn_desc(16, 64, 32, C0=36)),
        ("gn_ld0_not_multiple_of_8", N.gn_desc(16, 64, 32, ld0=68)),
        ("gn_ld1_not_multiple_of_8", N.gn_desc(16, 128, 32, C0=64, ld1=68)),
        ("gn_ldy_not_multiple_of_8", N.gn_desc(16, 64, 32, ldy=68)),
        ("gn_stats_c_not_multiple_of_groups", N.gn_desc(16, 64, 48, mode="GN_STATS")),
        ("gn_stats_ld_not_multiple_of_8", N.gn_desc(16, 64, 32, mode="GN_STATS", ld0=68)),
        ("gn_finalize_c_not_multiple_of_groups", N.gn_desc(16, 64, 48, mode="GN_FINALIZE", nslab=1)),
        ("ln_c_not_multiple_of_8", N.ln_desc(5, 12)),
        ("ln_c_above_2048", N.ln_desc(5, 2056)),
        ("ln_ldx_not_multiple_of_8", N.ln_desc(5, 64, ldx=68)),
        ("ln_ldy_not_multiple_of_8", N.ln_desc(5, 64, ldy=68)),
    ]


@pytest.mark.parametrize("name,d", _refusals(), ids=[r[0] for r in _refusals()])
def test_refused_launches_leave_the_outputs_untouched(ctx, name, d):
    r = np.random.default_rng(3)
    ext = N.extents(d)
    ops = {s: (r.standard_normal(ext[s]).astype(np.float16 if s in ("X0", "X1") else np.float32)) for s in N.INPUTS if ext[s]}
    rc, outs, info = run(ctx, d, ops)
    assert rc != 0, f"{name} was not refused"
    assert all(v == 0 for v in info.values()), info
    replay.assert_untouched(outs, name)


# ---- the product's own graphs reach the paths the sweep checks ----------------------------------------------------------------------
def _path_counts(ctx, reset=0):
    c = np.zeros(8, np.int64)
    assert replay.lib().tsd_debug_gn_path_counts(ctx.h, c.ctypes.data_as(_i64p), 8, reset) == 0
    return dict(zip(("all", "own", "table", "table_finalize", "prereduce", "composite", "finalize", "composite_offered"), map(int, c)))


def test_production_graphs_reach_every_groupnorm_path(ctx, tsd_mod):
    """One UNet forward at a 16 x 16 latent and one decoder forward at a 16 x 16 latent (128 x 128 images: 512 producer slabs, the
    smallest the decoder takes above 256), counted per path by the plan launch_groupnorm itself acts on."""
    rng = np.random.default_rng(SEED)
    _path_counts(ctx, reset=1)
    unet = tsd_mod.Diffusion(seed=SEED, ctx=ctx)
    try:
        unet.forward(*(rng.standard_normal(s).astype(np.float32) for s in ((1, 4, 16, 16), (1, 77, 768), (1, 320))))
    finally:
        unet.model.close()
    u = _path_counts(ctx, reset=1)
    dec = tsd_mod.Decoder(seed=SEED, ctx=ctx)
    try:
        dec.forward(rng.standard_normal((1, 4, 16, 16)).astype(np.float32))
    finally:
        dec.model.close()
    v = _path_counts(ctx, reset=1)
    print(f"\n[norm] GroupNorm launches per path: UNet 16x16 {u}\n[norm]                              decoder 16x16 {v}")
    assert u["all"] > 20 and v["all"] > 20
    assert u["own"] + v["own"] > 0, "no launch ran its own statistics pass"
    assert u["table"] + v["table"] > 0, "no producer table was finished inside the apply blocks"
    assert u["table_finalize"] + v["table_finalize"] > 0, "no producer table was finished by the finalize launch"
    assert v["prereduce"] > 0, "the decoder's large images did not prereduce"
    assert u["composite"] > 0 and u["composite"] <= u["composite_offered"], "the UNet's concat inputs accepted no composite"
