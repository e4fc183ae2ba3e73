"""UNet layer 10 reads concat(x, x) of ONE tensor (diffusion.mojo:253-256).  With TSD_FOLD_DUP (default) tsd_model_prepare adds the two
input-channel halves of its conv1 / skip weights on the host - exact sum, one nearest-even rounding to fp16 (tests/test_dup_fold_cpu.py
holds that arithmetic to numpy) - and the block runs as 1280 -> 1280 with GroupNorm(16), whose statistics are the bottleneck's 32-group
partials added in pairs: the very sums GroupNorm(32) over [x | x] makes for either half.

What is held here: the folded weights on the device are bit-equal to the numpy sum of the model's parameters (with test_gpu_gemm_ref.py,
which replays every recorded production launch against fp64, the folded layer then deviates from exact arithmetic by ONE correctly
rounded fp16 rounding per weight - no tolerance needed for that statement); the model stays inside the oracle's tolerance with the
fold on and off, the two differ, and agree within the project's bound for a weight fold (2e-3, as for the GEGLU-2 / conv_out fold);
the launches are the ones the issue names and no statistics pass was added; batch invariance, refolding after set_param, and the
refusal of a sum that leaves fp16."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oracle import models, ops, rng
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, rel_l2

pytestmark = pytest.mark.gpu
SEED = 1234
W1, WSK = "unet.layer10.layer2.kernel", "unet.layer10.layer6.kernel"
_i64p = C.POINTER(C.c_int64)


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


@pytest.fixture(scope="module")
def ctx_off(gpu_ctx):
    from tsd._lib import Context
    with _env("TSD_FOLD_DUP", "0"):  # read once, by tsd_ctx_create
        c = Context(gpu_ctx.device)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_on(gpu_ctx):
    """the fold stated, not inherited: these tests hold whichever way the default points"""
    from tsd._lib import Context
    with _env("TSD_FOLD_DUP", "1"):
        c = Context(gpu_ctx.device)
    yield c
    c.close()


@pytest.fixture(scope="module")
def unet_on(ctx_on, tsd_mod):
    d = tsd_mod.Diffusion(seed=SEED, ctx=ctx_on)
    yield d
    d.model.close()


@pytest.fixture(scope="module")
def unet_off(ctx_off, tsd_mod):
    d = tsd_mod.Diffusion(seed=SEED, ctx=ctx_off)
    yield d
    d.model.close()


def _inputs(B, L, T=77, tag=1500):
    lat = rng.normal(SEED, tag, B * 4 * L * L).reshape(B, 4, L, L)
    ctx = rng.normal(SEED, tag + 1, B * T * 768).reshape(B, T, 768)
    temb = np.stack([ops.time_embedding(float((211 * (b + 1)) % 1000)) for b in range(B)])
    return lat, ctx, temb


def _lib(tsd_mod):
    return tsd_mod._lib.lib()


def _param_index(model, name):
    return [n for n, _, _, _ in model.specs].index(name)


def _numpy_fold(w):
    """OIHW fp32 parameter with I = 2 * half -> folded fp16 bits [O][taps][half], the packed layout (channel innermost)"""
    w16 = w.astype(np.float16).astype(np.float64)  # what the blob holds
    half = w.shape[1] // 2
    s = (w16[:, :half] + w16[:, half:]).astype(np.float16)
    return np.ascontiguousarray(s.transpose(0, 2, 3, 1)).reshape(w.shape[0], w.shape[2] * w.shape[3], half).view(np.uint16)


def _read_fold(tsd_mod, model):
    lib = _lib(tsd_mod)
    half = lib.tsd_debug_model_dup_fold(model.h, None, None)
    if half <= 0:
        return half, None, None
    w1 = np.empty((1280, 9, half), np.uint16)
    wsk = np.empty((1280, 1, half), np.uint16)
    assert lib.tsd_debug_model_dup_fold(model.h, w1.ctypes.data_as(C.c_void_p), wsk.ctypes.data_as(C.c_void_p)) == half
    return half, w1, wsk


def test_folded_weights_are_the_numpy_sum_of_the_parameters_bit_for_bit(tsd_mod, unet_on, unet_off, unet_params):
    half, w1, wsk = _read_fold(tsd_mod, unet_on.model)
    assert half == 1280
    assert np.array_equal(w1, _numpy_fold(unet_params[W1]))
    assert np.array_equal(wsk, _numpy_fold(unet_params[WSK]))
    assert _read_fold(tsd_mod, unet_off.model)[0] == 0, "a TSD_FOLD_DUP=0 context folded"


@pytest.mark.parametrize("B,L", [(2, 16), (1, 8)])
def test_forward_with_and_without_the_fold(B, L, unet_on, unet_off, unet_params):
    """layer 10 runs on 4 x 4 (L = 16) and 2 x 2 (L = 8) pixels"""
    lat, ctx, temb = _inputs(B, L, tag=1500 + L)
    ref = np.stack([models.diffusion(unet_params, lat[b], ctx[b], temb[b]) for b in range(B)])
    y1 = np.asarray(unet_on.forward(lat, ctx, temb), np.float32).reshape(ref.shape)
    y0 = np.asarray(unet_off.forward(lat, ctx, temb), np.float32).reshape(ref.shape)
    assert_close(y1, ref, TOL_MODEL, TOL_MODEL_MAX, f"Diffusion.forward B={B} L={L}, layer 10 folded")
    assert_close(y0, ref, TOL_MODEL, TOL_MODEL_MAX, f"Diffusion.forward B={B} L={L}, layer 10 over the concat")
    d = rel_l2(y1, y0)
    print(f"[parity] folded layer 10 vs the concat B={B} L={L}: rel_l2={d:.3e}")
    assert d > 0.0, "the two paths gave the same bits: the fold did not run"
    assert d <= 2e-3, d


def _account(tsd_mod, unet, lat, ctx, temb):
    c = unet.model.ctx
    counts = np.zeros(8, np.int64)
    unet.forward(lat, ctx, temb)  # derived buffers, arena
    assert _lib(tsd_mod).tsd_debug_gn_path_counts(c.h, counts.ctypes.data_as(_i64p), 8, 1) == 0
    c.profile_begin()
    try:
        unet.forward(lat, ctx, temb)
        recs = c.profile_records()
    finally:
        c.profile_end()
    assert _lib(tsd_mod).tsd_debug_gn_path_counts(c.h, counts.ctypes.data_as(_i64p), 8, 1) == 0
    gn = dict(zip(("all", "own", "table", "table_finalize", "prereduce", "composite", "finalize", "composite_offered"), map(int, counts)))
    return recs, gn


@pytest.mark.parametrize("B,L", [(2, 16), (1, 8)])
def test_launch_accounting(B, L, tsd_mod, unet_on, unet_off):
    lat, ctx, temb = _inputs(B, L, tag=1540 + L)
    on, gn_on = _account(tsd_mod, unet_on, lat, ctx, temb)
    off, gn_off = _account(tsd_mod, unet_off, lat, ctx, temb)
    conv_k = lambda recs, K: sum(1 for r in recs if r[0] == "conv3x3" and r[3] == K)  # noqa: E731
    gn_c = lambda recs, Cn: sum(1 for r in recs if r[0] == "groupnorm" and r[2] == Cn)  # noqa: E731
    print(f"[dup fold] B={B} L={L}: launches {len(on)} / {len(off)}, conv K=23040 {conv_k(on, 23040)} / {conv_k(off, 23040)}, "
          f"K=11520 {conv_k(on, 11520)} / {conv_k(off, 11520)}, GroupNorm C=2560 {gn_c(on, 2560)} / {gn_c(off, 2560)}\n"
          f"[dup fold] GroupNorm paths on {gn_on}\n[dup fold]                 off {gn_off}")
    assert conv_k(off, 23040) == 1 and gn_c(off, 2560) == 1, "the unfolded graph is not what this test assumes"
    assert conv_k(on, 23040) == 0, "a conv3x3 with K = 23040 ran with the fold on"
    assert gn_c(on, 2560) == 0, "a GroupNorm over 2560 channels ran with the fold on"
    assert conv_k(on, 11520) == conv_k(off, 11520) + 1
    assert len(on) == len(off)
    assert gn_on["all"] == gn_off["all"]
    assert gn_on["own"] == gn_off["own"], "the fold added (or removed) a statistics pass"
    assert gn_on["composite_offered"] - gn_on["composite"] == gn_off["composite_offered"] - gn_off["composite"]


def test_batch_invariance_is_bitwise_with_the_fold(unet_on):
    B, L = 3, 24
    lat, ctx, temb = _inputs(B, L, tag=1580)
    batched = unet_on.forward(lat, ctx, temb)
    assert np.isfinite(batched).all()
    np.testing.assert_array_equal(unet_on.forward(lat[B - 1], ctx[B - 1], temb[B - 1]), batched[B - 1])


def test_a_weight_set_after_prepare_is_refolded(tsd_mod, ctx_on, unet_params):
    """set_param invalidates the derived buffers: the next forward folds the NEW conv1, bit for bit what a model that never saw the
    old weight computes."""
    lat, ctx, temb = _inputs(1, 8, tag=1600)
    w = np.array(unet_params[W1], np.float32)
    w[3, 5, 1, 1] += 0.25; w[3, 1280 + 5, 1, 1] -= 0.125; w[700, 1279, 2, 0] = 0.5; w[700, 2559, 2, 0] = 2.0 ** -12
    a = tsd_mod.Diffusion(seed=SEED, ctx=ctx_on)
    b = tsd_mod.Diffusion(seed=SEED, ctx=ctx_on)
    try:
        before = np.array(a.forward(lat, ctx, temb))      # prepared with the old weight
        idx = _param_index(a.model, W1)
        a.model.set_param(idx, w)
        b.model.set_param(idx, w)                          # fresh: its first fold is of the new weight
        ya, yb = np.array(a.forward(lat, ctx, temb)), np.array(b.forward(lat, ctx, temb))
        half, w1, _ = _read_fold(tsd_mod, a.model)
    finally:
        a.model.close()
        b.model.close()
    assert half == 1280 and np.array_equal(w1, _numpy_fold(w))
    assert np.isfinite(ya).all() and not np.array_equal(ya, before), "the new weight changed nothing"
    np.testing.assert_array_equal(ya, yb)


def test_a_sum_that_leaves_fp16_is_refused_by_prepare(tsd_mod, ctx_on, ctx_off, unet_params):
    """40000 + 40000 = inf in fp16: tsd_model_prepare returns TSD_E_NONFINITE (-7) and names the layer; without the fold the same model
    prepares and runs."""
    w = np.array(unet_params[W1], np.float32)
    w[17, 33, 0, 2] = 40000.0; w[17, 1280 + 33, 0, 2] = 40000.0
    lib = _lib(tsd_mod)
    a = tsd_mod.Diffusion(seed=SEED, ctx=ctx_on)
    try:
        a.model.set_param(_param_index(a.model, W1), w)
        assert lib.tsd_model_prepare(a.model.h) == -7
        assert "layer10" in tsd_mod._lib.last_error()
        assert lib.tsd_model_prepare(a.model.h) == -7, "the refusal did not hold on the second call"
    finally:
        a.model.close()
    b = tsd_mod.Diffusion(seed=SEED, ctx=ctx_off)
    try:
        b.model.set_param(_param_index(b.model, W1), w)
        assert lib.tsd_model_prepare(b.model.h) == 0
        lat, ctx, temb = _inputs(1, 8, tag=1620)
        y = np.asarray(b.forward(lat, ctx, temb))
        assert y.shape[-3:] == (4, 8, 8)
    finally:
        b.model.close()
