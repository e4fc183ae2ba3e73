"""GPU: the attention core - flash_attn_kernel<40,1>, <40,2>, <80,1>, <160,1> (csrc/kernels_attn.hip), flash_attn8_kernel<40>
(csrc/kernels_attn8.hip) - and the row-softmax kernels of csrc/kernels_elementwise.hip held to an fp64 reference element-wise
(tests/attn_ref.py) through tsd_debug_attn_run: chosen Q / K / V^T bits, pitches wider than H*d, batch strides and a V^T pitch with
gaps, every kernel forced and by shape, the Sq / Sk edges of the loaders and of the tile loop, self-attention with the own-block
reference on and off, the XCD map, the score shapes of attn_ref (flat, equal keys, rising, spike, self-peaked, very low, one-hot,
subnormal tail, the overflow edge, a biased P rounding, a two-group score at 64 units), finite garbage in the V^T pad columns, and
the documented refusals.  Every case asserts the status, the kernel the launch reports, that no guard or pitch-gap element was
written, the exact-repeat prediction, and every output element against the bound; it prints the worst error / bound.

Worst error / bound seen on an MI355X, kernels 40/1, 40/2, 40/8-wave, 80, 160: Sq sweep 0.181 0.181 0.181 0.153
0.093; Sk sweep 0.461 0.461 0.461 0.414 0.269; self-peaked 0.006 0.006 0.006 0.000 0.000; equal keys 0.015 0.015 0.015 0.013 0.010; rising
0.012 0.012 0.013 0.017 0.016; rising, partial last tile 0.035 0.035 0.036 0.042 0.044; spike 0.097 0.097 0.095 0.134 0.114; scores near
-300 0.000; one-hot 0.326 0.326 0.320 0.348 0.329; subnormal tail 0.218 0.218 0.213 0.218 0.170; overflow edge 0.038 0.038 0.038 0.044
0.085; biased P rounding 0.000 (d = 40, 80: it cancels) and 0.550 (d = 160); two groups at 64 units 0.105 0.105 0.101 0.077 0.100; by
shape 0.128 0.096 0.071 (d = 40, 80, 160); XCD map 0.117 (d = 40) 0.064 (d = 80).  No case fell into the "may" band of the exact-repeat
prediction.  Row softmax: fp16 0.999 (one fp16 rounding: an output half an ulp from the reference sits at the bound by construction), fp32
0.300.

Dispatcher mode 0 on H = 8, Sq = 4096 (the shape at which it picks the 8-wave / 64-query kernels) is asserted through the sizing call
only (tests/test_attn_ref_cpu.py): its fp64 reference is too large for a test of a few seconds; here mode 0 runs at a small shape."""
import numpy as np
import pytest

import attn_ref as A
import replay

pytestmark = pytest.mark.gpu
SWEEP = A.sweep()
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
    p = A.plan(d, attn_xcd=xcd)
    assert {k: info[k] for k in p} == p, f"{name}: the launch took another path: {info}, expected {p}"
    assert info["CHANGED"] == 0, f"{name}: {info['CHANGED']} guard / pitch-gap elements written"
    replay.assert_gaps_hold_fill(out, A.o_index(d), f"{name}: O")
    pr = A.predict_repeat(d, ops)
    must, may = int((pr == 1).sum()), int((pr == 0).sum())
    fails, ratio = A.check(d, ops, out, ref=ref)
    print(f"[attn] {name}: worst error / bound {ratio:.3f}  kernel {A.KERNEL_NAME[info['KERNEL']]} diag {info['DIAG']} xcd {info['XCD_MAP']} "
          f"exact repeats {info['EXACT_WGS']} (must {must}, may {may} more, of {pr.size})")
    assert must <= info["EXACT_WGS"] <= must + may, f"{name}: {info['EXACT_WGS']} workgroups repeated, prediction {pr.tolist()}"
    assert not fails, f"{name}: " + "; ".join(fails)
    return out, info, ratio


# ---- every kernel over the Sq / Sk edges and the score shapes ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_attention_kernel_matches_the_fp64_reference(ctx, name):
    d, kind, ops, ref = A.case(name)
    if kind != "onehot":
        assert A.well_conditioned(d, ops)
    out, info, _ = verify(ctx, name, d, ops, ref)
    if kind == "equal":        # equal keys give equal score bits: every P is the same number, the ones-row sum is the count times it and the
        v = A.unpack_inputs(d, ops)[2].astype(np.float64)          # output the mean of V - to the fp32 accumulation and one fp16 rounding
        y = A.unpack_output(d, out).astype(np.float64)
        mean, g = v.mean(axis=2, keepdims=True), A._gamma(65 * -(-A.F(d, "SK") // 64) + 2) + 5 * A.U32
        assert (np.abs(y - mean) <= (A.H16 + 4 * g) * (np.abs(v).mean(axis=2, keepdims=True) + np.abs(mean)) + 2.0 ** -25).all()


def test_dispatcher_by_shape_at_a_small_shape(ctx):
    for hd, kern in ((40, "40_1"), (80, "80"), (160, "160")):
        d = A.attn_desc(2, 3, hd, 129, 129, kernel=0)
        ops = A.make_inputs(d, "flat", seed=9)
        _, info, _ = verify(ctx, f"mode0/d{hd}", d, ops)
        assert info["KERNEL"] == A.AK[kern] and info["DIAG"] == 1


# ---- the XCD map ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", (40, 80))
def test_xcd_map_gives_the_same_bits(ctx, gpu_ctx, tsd_mod, monkeypatch, hd):
    c = replay.ctx_with(tsd_mod, gpu_ctx, monkeypatch, "TSD_ATTN_XCD", 1)
    try:
        for mode in ((1, 2, 3) if hd == 40 else (0,)):
            d = A.attn_desc(2, 8, hd, 256, 512, kernel=mode)
            ops = A.make_inputs(d, "flat", seed=13)
            ref = A.reference(d, ops)
            y0, i0, _ = verify(ctx, f"xcd0/d{hd}/mode{mode}", d, ops, ref)
            y1, i1, _ = verify(c, f"xcd1/d{hd}/mode{mode}", d, ops, ref, xcd=1)
            assert i0["XCD_MAP"] == 0 and i1["XCD_MAP"] == 1
            assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16)), "the XCD map changed a bit of the output"
    finally:
        c.close()


# ---- V^T pad columns ---------------------------------------------------------------------------------------------------------------
PADS = A.pad_sweep()


@pytest.mark.parametrize("name,d", PADS, ids=[p[0] for p in PADS])
def test_finite_pad_columns_of_vt_do_not_change_a_bit(ctx, name, d):
    """V^T columns [Sk, Skv) reach the P.V MFMA with P = 0: any finite content gives the same bits.  Columns >= Skv, the K pitch gap and
    the batch gaps hold the NaN pattern in both runs and are never read."""
    z = A.make_inputs(d, "flat", seed=7, pad=0.0)
    f = A.make_inputs(d, "flat", seed=7, pad=A.pad_fill(d))
    assert A.skv_of(d) > A.F(d, "SK") and not np.array_equal(z["VT"].view(np.uint16), f["VT"].view(np.uint16))
    assert np.isnan(z["VT"]).any() and np.isnan(z["K"]).any()
    ref = A.reference(d, z)
    y0, _, _ = verify(ctx, name + "/zero", d, z, ref)
    y1, _, _ = verify(ctx, name + "/60000", d, f, ref)
    assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16)), f"{name}: the V^T pad columns reached the output"


def test_public_cross_attention_at_77_keys_does_not_read_the_arena(gpu_ctx, tsd_mod, monkeypatch):
    """The context V^T of tsd_cross_attention_f32 has pitch 80 at T = 77: its columns 77 .. 79 come from the zero rows the context is
    padded with, not from what the arena held - the result is finite and does not change with the byte fresh arena memory is filled
    with (0x7E7E is an fp16 NaN)."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((64, 320)).astype(np.float32)
    context = rng.standard_normal((77, 768)).astype(np.float32)
    m = tsd_mod.Cross_Attention(8, 320, 768, seed=3)      # one set of weights; only the context differs
    ys = []
    for byte in (0x7E, 0x00):
        m.ctx = replay.ctx_with(tsd_mod, gpu_ctx, monkeypatch, "TSD_DEBUG_POISON", byte)
        try:
            ys.append(m.forward(x, context))
        finally:
            m.ctx.close()
    assert np.isfinite(ys[0]).all()
    assert np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32)), "the result depends on what the arena held"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _refusals():
    return [
        ("head_dim_48", A.attn_desc(1, 2, 48, 8, 16)),
        ("head_dim_64", A.attn_desc(1, 1, 64, 8, 16)),
        ("ldq_not_multiple_of_8", A.attn_desc(1, 2, 40, 8, 16, ldq=84)),
        ("ldk_not_multiple_of_8", A.attn_desc(1, 2, 40, 8, 16, ldk=84)),
        ("ldvt_not_multiple_of_8", A.attn_desc(1, 2, 40, 8, 16, ldvt=20)),
        ("ldo_not_multiple_of_4", A.attn_desc(1, 2, 40, 8, 16, ldo=82)),
        ("empty_queries", A.attn_desc(1, 2, 40, 0, 16)),
        ("empty_keys", A.attn_desc(1, 2, 40, 8, 0)),
    ]


@pytest.mark.parametrize("name,d", _refusals(), ids=[r[0] for r in _refusals()])
def test_refused_launches_leave_the_output_untouched(ctx, name, d):
    r = np.random.default_rng(3)
    ext = A.extents(d)
    ops = {s: r.standard_normal(ext[s]).astype(np.float16) for s in ("Q", "K", "VT")}
    rc, out, info = run(ctx, d, ops)
    assert rc != 0, f"{name} was not refused"
    assert all(v == 0 for v in info.values()), info
    replay.assert_untouched({"O": out}, name)


# ---- row softmax -------------------------------------------------------------------------------------------------------------------
SM_SWEEP = A.softmax_sweep()


@pytest.mark.parametrize("name,d", SM_SWEEP, ids=[s[0] for s in SM_SWEEP])
def test_softmax_rows_match_the_fp64_reference(ctx, name, d):
    x = A.softmax_inputs(d, seed=5)
    rc, out, info = run(ctx, d, {"X": x})
    assert rc == 0, replay.lib().tsd_last_error().decode()
    assert info["KERNEL"] == A.softmax_kernel(d), f"{name}: the launcher took kernel {info['KERNEL']}"
    assert info["CHANGED"] == 0, f"{name}: {info['CHANGED']} guard / pitch-gap elements written"
    fails, ratio = A.softmax_check(d, x, out)
    print(f"[attn] softmax {name}: worst error / bound {ratio:.3f}  kernel {info['KERNEL']}")
    assert not fails, f"{name}: " + "; ".join(fails)
    rows = A._softmax_rows_of(d, out, A.F(d, "COLS")).astype(np.float64)
    assert np.abs(rows.sum(axis=1) - 1).max() < 2e-2
