"""The upsample fold (TSD_UPS_FOLD): conv1 of the residual blocks behind a nearest-2x upsample (UNet layers 15 and 20) executes
K = 4 Cin on four 2x2 parity kernels whose weights tsd_model_prepare summed from the 3x3 ones (tests/test_ups_fold_cpu.py holds that
arithmetic and the algebra).

What is held here: (1) the kernel variant, through tsd_debug_gemm_run with UPS = 2, against a float64 statement of what it executes -
the gathered 2x2 source pixels times the numpy-folded, fp16-rounded weights - on ALL rows and columns, within gemm_ref.bound for
K = 4 Cin, for every tile configuration that has the variant; (2) the refusals, which must leave the outputs as they were; (3) the
graph: oracle tolerance with the option on and off, the on-against-off distance, bitwise batch invariance across tile
configurations, the recorded descriptors and GroupNorm paths of a production step, the device copy of the folded weights bit for bit,
refolding after set_param, and the refusal of a sum that leaves fp16.  With test_gpu_gemm_ref.py, which replays every recorded
production launch (UPS = 2 included) against the fp64 3x3 reference with the ORIGINAL weights, that covers the path end to end."""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as G
import replay
import ups_fold_ref as U
from oracle import models, ops, rng
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, rel_l2

pytestmark = pytest.mark.gpu
E = G.EPI
SEED = 1234
UF_CFGS = (0, 1, 5, 6, 7, 51)      # tile configurations that have the variant (kernels_gemm.hip launch_ups_fold)
BLOCKS = {14: "unet.layer15.layer2.kernel", 19: "unet.layer20.layer2.kernel"}   # residual block index -> its conv1 parameter
_i64p = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def ctx(gpu_ctx, tsd_mod):
    c = tsd_mod.Context(gpu_ctx.device)
    assert replay.lib().tsd_debug_set_ups_fold(c.h, 1) in (0, 1)   # stated, not inherited
    yield c
    c.close()


def run(ctx, d, ops_, cfg=-1):
    """(status, outputs, info [cfg, ways, guard / gap writes]); a descriptor the entry cannot size returns (status, None, None)"""
    return replay.run("tsd_debug_gemm_run", ctx, d, ops_, G.GO, G.INPUTS, G.OUTPUTS, G.dtype_of, G.extents, extra=(cfg,), unsizable_ok=True)


# ---- (1) the kernel against float64, with the folded weights -------------------------------------------------------------------
def _desc(B, Hs, Ws, Cin, N, **f):
    f.setdefault("epi", E["BIAS_N"] | E["ROWVEC"])
    d = G.conv_desc(B, Hs, Ws, Cin, N, ups=2, rps_hint=4 * Hs * Ws, **f)
    if int(d[G.GD["EPI"]]) & E["ROWVEC"]:
        d[G.GD["ROWVEC_LD"]] = N
        d[G.GD["ROWS_PER_BATCH"]] = 4 * Hs * Ws       # = Ho * Wo: one row vector per sample
    return d


def _expected(d, ops_):
    """(v, bound) [M][N] in output-pixel row order: what the launch executes, in float64 - for parity q the gathered 2x2 source pixels
    times the folded fp16 weights - plus bias and row vector; the bound is gemm_ref's for K = 4 Cin"""
    g = lambda k: int(d[G.GD[k]])   # noqa: E731
    Hs, Ws, Ho, Wo, Cin, N, M, lda = g("HS"), g("WS"), g("HO"), g("WO"), g("CIN"), g("N"), g("M"), g("LDA0")
    B, K4 = M // (Ho * Wo), 4 * Cin
    a = np.zeros(B * Hs * Ws * lda, np.float16)
    a[:ops_["A0"].size] = ops_["A0"]
    x = a.reshape(B, Hs, Ws, lda)[..., :Cin].astype(np.float64)
    assert np.isfinite(x).all()
    w = ops_["W"]
    W9 = w.reshape(N, 9 * Cin) if g("W_KTS") else w[np.arange(N)[:, None] * g("LDW") + np.arange(9 * Cin)[None, :]]
    f16 = U.fold16(W9.reshape(N, 3, 3, Cin))
    assert np.isfinite(f16).all()
    f = f16.astype(np.float64)
    acc = np.empty((B, Ho, Wo, N))
    sabs = np.empty((B, Ho, Wo, N))
    for q in range(4):
        A = U.gather2x2(x, q)
        Wq = f[q].reshape(N, K4)
        acc[:, (q >> 1)::2, (q & 1)::2] = A @ Wq.T
        sabs[:, (q >> 1)::2, (q & 1)::2] = np.abs(A) @ np.abs(Wq).T
    acc, sabs = acc.reshape(M, N), sabs.reshape(M, N)
    v, mag, terms = acc.copy(), sabs.copy(), 0
    e = 2 * K4 * G.U32 * sabs + G.U32 * sabs
    epi = g("EPI")
    if epi & E["BIAS_N"]:
        t = ops_["BIAS"].astype(np.float64)[None, :N]
        v, mag, terms = v + t, mag + np.abs(t), terms + 1
    if epi & E["ROWVEC"]:
        rv = ops_["ROWVEC"].astype(np.float64)
        t = rv[(np.arange(M) // g("ROWS_PER_BATCH"))[:, None] * g("ROWVEC_LD") + np.arange(N)[None, :]]
        v, mag, terms = v + t, mag + np.abs(t), terms + 1
    e = e + (terms + 1) * G.U32 * mag
    return v, G.bound(d, v, e)


def _hold(d, outs, info, v, bnd, what):
    assert info[2] == 0, f"{what}: {info[2]} guard / pitch-gap elements written"
    M, N, ldc = (int(d[G.GD[k]]) for k in ("M", "N", "LDC"))
    got = outs["C"][np.arange(M)[:, None] * ldc + np.arange(N)[None, :]].astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements not written or not finite"
    err = np.abs(got - v)
    worst = float((err / bnd).max())
    print(f"[ups fold] {what}: cfg {int(info[0])} ways {int(info[1])}, worst error / bound {worst:.3f}")
    assert (err <= bnd).all(), f"{what}: {int((err > bnd).sum())} elements beyond the bound, worst {worst:.3f} at {np.argwhere(err > bnd)[:4].tolist()}"


SHAPES = {
    # two samples, square plane of 256 pixels: 256-row tiles hold exactly one parity plane, tile row blocks change sample and parity
    "b2_16x16_c64": dict(B=2, Hs=16, Ws=16, Cin=64, N=320),
    # Hs != Ws, two channel chunks per tap (the tap / chunk cursor wraps), pitches wider than the rows with NaN in the gaps, K-tile-major W described
    "8x32_c128_pitch": dict(B=1, Hs=8, Ws=32, Cin=128, N=160, lda0=128 + 8, ldc=160 + 8, w_kts=1),
}


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, (name, s) in enumerate(SHAPES.items()):
        d = _desc(**s)
        ops_ = G.make_operands(d, 900 + i)
        out[name] = (d, ops_) + _expected(d, ops_)
    return out


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("cfg", UF_CFGS)
def test_every_configuration_with_the_variant_against_fp64(ctx, cases, name, cfg):
    d, ops_, v, bnd = cases[name]
    rc, outs, info = run(ctx, d, ops_, cfg)
    assert rc == 0, replay.lib().tsd_last_error().decode()
    assert int(info[0]) == cfg and int(info[1]) == 1
    _hold(d, outs, info, v, bnd, f"{name} forced {cfg}")


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_dispatchers_choice_twice_with_equal_bits(ctx, cases, name):
    d, ops_, v, bnd = cases[name]
    rc, outs, info = run(ctx, d, ops_)
    assert rc == 0, replay.lib().tsd_last_error().decode()
    assert int(info[0]) in UF_CFGS and int(info[1]) == 1
    _hold(d, outs, info, v, bnd, f"{name} dispatcher")
    rc2, outs2, info2 = run(ctx, d, ops_)
    assert rc2 == 0 and (info2[:3] == info[:3]).all()
    assert np.array_equal(outs["C"].view(np.uint16), outs2["C"].view(np.uint16))


def test_row_major_description_and_no_row_vector(ctx, cases):
    """the same weights described row-major with a wider pitch (W_KTS off, ldw > 9 Cin) and a bias-only epilogue"""
    s = dict(SHAPES["8x32_c128_pitch"], w_kts=0, epi=E["BIAS_N"])
    d = _desc(**s)
    d[G.GD["LDW"]] = 9 * 128 + 16
    ops_ = G.make_operands(d, 950)
    v, bnd = _expected(d, ops_)
    rc, outs, info = run(ctx, d, ops_)
    assert rc == 0, replay.lib().tsd_last_error().decode()
    _hold(d, outs, info, v, bnd, "row-major W, bias only")


# ---- (2) refusals write nothing -------------------------------------------------------------------------------------------------
def _refused(ctx, d, cfg=-1, seed=970):
    ops_ = G.make_operands(d, seed)
    rc, outs, info = run(ctx, d, ops_, cfg)
    assert rc != 0, "the launch was accepted"
    if outs is None:
        return "sizing"     # refused before any buffer existed
    assert info[2] == 0
    replay.assert_untouched(outs, "a refused launch")
    return replay.lib().tsd_last_error().decode()


def test_refusals_leave_the_outputs_untouched(ctx):
    base = dict(B=1, Hs=16, Ws=16, Cin=64, N=320)
    # statistics: a one-parity tile holds no 32-raster-row slab
    d = _desc(**base, epi=E["BIAS_N"] | E["GNSTATS"])
    d[G.GD["GN_GROUPS"]], d[G.GD["GN_RPS"]], d[G.GD["GN_NSLAB"]] = 32, 1024, 32
    _refused(ctx, d)
    # stride 2
    _refused(ctx, _desc(**base, stride=2))
    # a fused skip: at stride 1 its sources cannot even be sized against the upsampled output; at stride 2 (Ho = Hs) the launch refuses it
    assert _refused(ctx, _desc(**base, Cin1=64)) == "sizing"
    _refused(ctx, _desc(**base, stride=2, Cin1=64))
    # residual / fp32 epilogues
    _refused(ctx, _desc(**base, epi=E["BIAS_N"] | E["RESIDUAL"]))
    _refused(ctx, _desc(**base, epi=E["BIAS_N"] | E["OUT_F32"]))
    # a source plane of 64 pixels: a 128-row tile would straddle two parities
    _refused(ctx, _desc(B=4, Hs=8, Ws=8, Cin=64, N=320))
    # Cin that is no whole K tile per tap is refused by conv3x3 itself; a width outside the 160-column tile family by the rule
    _refused(ctx, _desc(B=1, Hs=16, Ws=16, Cin=64, N=256))
    # forced configurations without the variant
    for cfg in (2, 45, 11, 24):
        assert "variant" in _refused(ctx, _desc(**base), cfg)
    # ... and the same description with UPS = 1 runs
    d = _desc(**base)
    d[G.GD["UPS"]] = 1
    rc, outs, info = run(ctx, d, G.make_operands(d, 971))
    assert rc == 0 and np.isfinite(outs["C"]).all()


# ---- (3) in the graph --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unet(ctx, tsd_mod):
    d = tsd_mod.Diffusion(seed=SEED, ctx=ctx)
    yield d
    d.model.close()


class _fold:
    """with _fold(ctx, on): the option for the block, the previous value back afterwards"""
    def __init__(self, ctx, on):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        self.prev = replay.lib().tsd_debug_set_ups_fold(self.ctx.h, self.on)
        assert self.prev in (0, 1)

    def __exit__(self, *a):
        replay.lib().tsd_debug_set_ups_fold(self.ctx.h, self.prev)


def _inputs(B, L, T=77, tag=1700):
    lat = rng.normal(SEED, tag, B * 4 * L * L).reshape(B, 4, L, L)
    cond = rng.normal(SEED, tag + 1, B * T * 768).reshape(B, T, 768)
    temb = np.stack([ops.time_embedding(float((211 * (b + 1)) % 1000)) for b in range(B)])
    return lat, cond, temb


def _param_index(model, name):
    return [n for n, _, _, _ in model.specs].index(name)


def _numpy_fold_tm(w):
    """OIHW fp32 parameter -> the device copy: fp16 bits [4][4 I / 64][O][64]"""
    w16 = np.ascontiguousarray(w.astype(np.float16).transpose(0, 2, 3, 1))   # what the blob holds, [O][3][3][I]
    return U.tile_major(U.fold16(w16)).view(np.uint16)


def _read_fold(model, block, O, I):
    lib = replay.lib()
    n = lib.tsd_debug_model_ups_fold(model.h, block, None)
    if n <= 0:
        return n, None
    out = np.empty((4, 4 * I // 64, O, 64), np.uint16)
    assert n == I and lib.tsd_debug_model_ups_fold(model.h, block, out.ctypes.data_as(C.c_void_p)) == I
    return n, out


def test_set_option_returns_the_previous_value(ctx):
    lib = replay.lib()
    assert lib.tsd_debug_set_ups_fold(ctx.h, 0) == 1
    assert lib.tsd_debug_set_ups_fold(ctx.h, 1) == 0
    assert lib.tsd_debug_set_ups_fold(ctx.h, 1) == 1
    assert lib.tsd_debug_set_ups_fold(None, 1) < 0


def test_folded_weights_on_the_device_are_the_numpy_fold_bit_for_bit(unet, unet_params):
    for block, name in BLOCKS.items():
        w = unet_params[name]
        n, got = _read_fold(unet.model, block, w.shape[0], w.shape[1])
        assert n == w.shape[1], f"block {block} did not fold"
        assert np.array_equal(got, _numpy_fold_tm(w)), f"block {block}"
    assert replay.lib().tsd_debug_model_ups_fold(unet.model.h, 9, None) == 0, "a block without an upsample folded"


def test_forward_inside_the_oracle_tolerance_with_the_fold_on_and_off(ctx, unet, unet_params):
    """L = 32: layer 20 folds (256-pixel source plane), layer 15 (64 pixels) runs the nine taps"""
    B, L = 2, 32
    lat, cond, temb = _inputs(B, L)
    ref = np.stack([models.diffusion(unet_params, lat[b], cond[b], temb[b]) for b in range(B)])
    with _fold(ctx, 1):
        y1 = np.asarray(unet.forward(lat, cond, temb), np.float32).reshape(ref.shape)
    with _fold(ctx, 0):
        y0 = np.asarray(unet.forward(lat, cond, temb), np.float32).reshape(ref.shape)
    assert_close(y1, ref, TOL_MODEL, TOL_MODEL_MAX, "Diffusion.forward B=2 L=32, upsample fold on")
    assert_close(y0, ref, TOL_MODEL, TOL_MODEL_MAX, "Diffusion.forward B=2 L=32, upsample fold off")
    d = rel_l2(y1, y0)
    print(f"[ups fold] on against off, B=2 L=32: rel_l2 = {d:.3e}")
    assert d > 0.0, "the two paths gave the same bits: the fold did not run"
    assert d < 2e-3, d


def test_batch_invariance_is_bitwise_with_the_fold(ctx, unet):
    with _fold(ctx, 1):
        lat, cond, temb = _inputs(3, 32, tag=1720)
        batched = unet.forward(lat, cond, temb)
        assert np.isfinite(batched).all()
        np.testing.assert_array_equal(unet.forward(lat[0], cond[0], temb[0]), batched[0])
        # L = 64: both layers fold, and batch 1 runs other tile configurations than batch 8
        lat, cond, temb = _inputs(8, 64, tag=1730)
        batched = unet.forward(lat, cond, temb)
        assert np.isfinite(batched).all()
        np.testing.assert_array_equal(unet.forward(lat[0], cond[0], temb[0]), batched[0])


def _recorded_step(ctx, tsd_mod, unet, B, L):
    lib = replay.lib()
    lat, cond, _ = _inputs(B, L, tag=1740)
    counts = np.zeros(8, np.int64)
    s = tsd_mod.Session(unet.model, None, B, L, 77, cfg=False)
    try:
        s.set_schedule(1000, 2, 0)
        s.upload(lat.astype(np.float32), cond.astype(np.float32), None, None)
        assert lib.tsd_debug_gn_path_counts(ctx.h, counts.ctypes.data_as(_i64p), 8, 1) == 0
        lib.tsd_debug_gemm_record(ctx.h, 1)
        try:
            s.step(0)
            s.latents()
        finally:
            n = lib.tsd_debug_gemm_record(ctx.h, 0)
        assert lib.tsd_debug_gn_path_counts(ctx.h, counts.ctypes.data_as(_i64p), 8, 1) == 0
    finally:
        s.close()
    descs = []
    for i in range(n):
        d = np.zeros(G.COUNT, np.int64)
        assert lib.tsd_debug_gemm_recorded(ctx.h, i, d.ctypes.data_as(_i64p), G.COUNT) == G.COUNT
        descs.append(d)
    return descs, dict(zip(("all", "own", "table", "table_finalize", "prereduce", "composite", "finalize", "composite_offered"), map(int, counts)))


def test_recorded_production_step(ctx, tsd_mod, unet):
    g = lambda d, k: int(d[G.GD[k]])   # noqa: E731
    ups = lambda descs, u: [d for d in descs if g(d, "CONV") and g(d, "UPS") == u]   # noqa: E731
    with _fold(ctx, 1):
        on, gn_on = _recorded_step(ctx, tsd_mod, unet, 8, 64)
    with _fold(ctx, 0):
        off, gn_off = _recorded_step(ctx, tsd_mod, unet, 8, 64)
    print(f"[ups fold] B=8 L=64 step: {len(on)} / {len(off)} GEMM launches\n[ups fold] GroupNorm paths on  {gn_on}\n[ups fold] GroupNorm paths off {gn_off}")
    assert sorted((g(d, "M"), g(d, "N"), g(d, "CIN")) for d in ups(on, 2)) == [(8192, 640, 1280), (32768, 320, 640)]
    assert not ups(on, 1)
    for d in ups(on, 2):
        assert not g(d, "EPI") & E["GNSTATS"] and g(d, "K") == 9 * g(d, "CIN") and g(d, "CFG") in UF_CFGS and g(d, "WAYS") == 1
    assert sorted((g(d, "M"), g(d, "N"), g(d, "CIN")) for d in ups(off, 1)) == [(8192, 640, 1280), (32768, 320, 640)]
    assert not ups(off, 2)
    assert len(on) == len(off)
    assert gn_on["all"] == gn_off["all"]
    assert gn_on["own"] == gn_off["own"] + 2, "a folded conv1 emits no statistics: exactly its two consumer norms run their own pass"


def test_a_weight_set_after_prepare_is_refolded(ctx, tsd_mod, unet_params):
    name = BLOCKS[19]
    w = np.array(unet_params[name], np.float32)
    w[3, 5, 1, 1] += 0.25; w[3, 5, 1, 2] -= 0.125; w[300, 639, 2, 0] = 0.5; w[300, 639, 2, 1] = 2.0 ** -12
    lat, cond, temb = _inputs(1, 32, tag=1760)
    a = tsd_mod.Diffusion(seed=SEED, ctx=ctx)
    b = tsd_mod.Diffusion(seed=SEED, ctx=ctx)
    try:
        with _fold(ctx, 1):
            before = np.array(a.forward(lat, cond, temb))      # prepared with the old weight
            idx = _param_index(a.model, name)
            a.model.set_param(idx, w)
            b.model.set_param(idx, w)                           # fresh: its first fold is of the new weight
            ya, yb = np.array(a.forward(lat, cond, temb)), np.array(b.forward(lat, cond, temb))
        n, got = _read_fold(a.model, 19, w.shape[0], w.shape[1])
    finally:
        a.model.close()
        b.model.close()
    assert n == w.shape[1] and np.array_equal(got, _numpy_fold_tm(w))
    assert np.isfinite(ya).all() and not np.array_equal(ya, before), "the new weight changed nothing"
    np.testing.assert_array_equal(ya, yb)


def test_a_sum_that_leaves_fp16_is_refused_by_prepare(ctx, tsd_mod, unet_params):
    """30000 + 30000 + 30000 in kernel rows {1, 2} of one column = inf in fp16: tsd_model_prepare returns TSD_E_NONFINITE (-7)"""
    name = BLOCKS[14]
    w = np.array(unet_params[name], np.float32)
    w[17, 33, 1, 0] = 30000.0; w[17, 33, 2, 0] = 30000.0; w[17, 33, 1, 1] = 30000.0
    lib = replay.lib()
    a = tsd_mod.Diffusion(seed=SEED, ctx=ctx)
    try:
        a.model.set_param(_param_index(a.model, name), w)
        assert lib.tsd_model_prepare(a.model.h) == -7
        assert "folded conv1" in tsd_mod._lib.last_error()
        assert lib.tsd_model_prepare(a.model.h) == -7, "the refusal did not hold on the second call"
    finally:
        a.model.close()
