"""GPU tests of the workspace rule (DESIGN.md "Workspace rule"): the context's arena and staging buffer are per-call scratch, and every pad a
kernel may read is written by the call that reads it.  The kernel tests show that FINITE values in those pads change no bit; these tests
show that the graphs make them finite, for every entry point that runs device work in the arena.

The whole check is bit equality - there is no tolerance.  `hold` runs a callable on the same context and the same models
  (a) after tsd_debug_scribble(0x00),
  (b) after scribble(0xFF): fp16 NaN, fp32 NaN, int -1,
  (c) after scribble(0x7B): fp16 61280, fp32 about 1.3e36 - large and finite,
  (d) after a donor call of another model and shape and no scribble (a decoder forward at L = 8 writes fp32 and fp16 all over the arena),
and requires the four results to be finite and equal as uint32 / uint16 bit patterns.  (d) is the production case, (b) the strict one.
The sessions are scribbled between every two calls, and the fresh-allocation side of the same statement (TSD_DEBUG_POISON, the session's
own growable buffers and the staging buffer included) is held on two contexts created with the bytes 0x00 and 0xFF.

A new graph adds its row here."""
import numpy as np
import pytest

import replay
from cases import _attn_params, _res_params, _w
from oracle import rng
from util import randn

pytestmark = pytest.mark.gpu
SEED = 1234
T = 77
CONDITIONS = (("a: scribble 0x00", 0x00), ("b: scribble 0xFF", 0xFF), ("c: scribble 0x7B", 0x7B), ("d: donor call, no scribble", None))


# ---- the helper ----------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).ravel()


def _arrays(result):
    return [np.asarray(r) for r in result] if isinstance(result, (list, tuple)) else [np.asarray(result)]


def _first(mask):
    return int(np.flatnonzero(mask.ravel())[0])


def compare(results, what):
    """results: [(condition name, [arrays])]; all finite, and every condition equal to the first one bit for bit."""
    for name, arrs in results:
        for k, a in enumerate(arrs):
            bad = ~np.isfinite(a)
            assert not bad.any(), f"{what}: condition ({name}): output {k} is not finite, first at flat index {_first(bad)} of {a.size} ({int(bad.sum())} in all)"
    name0, ref = results[0]
    for name, arrs in results[1:]:
        assert len(arrs) == len(ref)
        for k, (a, r) in enumerate(zip(arrs, ref)):
            assert a.shape == r.shape and a.dtype == r.dtype, (what, name, k)
            diff = _bits(a) != _bits(r)
            assert not diff.any(), (f"{what}: condition ({name}) differs from ({name0}) in output {k}: first at flat index {_first(diff)} of {a.size} "
                                    f"({int(diff.sum())} elements differ; {a.ravel()[_first(diff)]!r} against {r.ravel()[_first(diff)]!r})")


def hold(tsd_mod, ctx, donor, fn, what):
    """fn() under the four conditions.  One unchecked donor + fn pair comes first: it sizes the arena and the staging buffer (a scribble
    covers what is allocated when it runs) and builds what a model derives on its first forward."""
    try:
        donor()
        fn()
    except tsd_mod.TsdError as e:
        pytest.fail(f"{what}: the first call, on what the tests before it left in the workspace: {e}")
    results = []
    for name, byte in CONDITIONS:
        if byte is not None:
            ctx.scribble(byte)
        try:
            if byte is None:
                donor()
            results.append((name, _arrays(fn())))
        except tsd_mod.TsdError as e:
            pytest.fail(f"{what}: condition ({name}): {e}")
    compare(results, what)


class option:
    """One tsd_debug_set_* switch of the shared context at `value` inside the block; restored on exit."""

    def __init__(self, tsd_mod, ctx, name, value):
        self.fn, self.h, self.value = getattr(tsd_mod._lib.lib(), "tsd_debug_set_" + name), ctx.h, int(value)

    def __enter__(self):
        self.prev = self.fn(self.h, self.value)
        assert self.prev in (0, 1), self.prev

    def __exit__(self, *exc):
        self.fn(self.h, self.prev)


def _normal(tag, *shape):
    return rng.normal(SEED, tag, int(np.prod(shape))).reshape(shape).astype(np.float32)


# ---- models (seeded on the device) and the donors --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(gpu_ctx, tsd_mod):
    d = tsd_mod.Diffusion(seed=SEED)
    yield d
    d.model.close()


@pytest.fixture(scope="module")
def decoder(gpu_ctx, tsd_mod):
    d = tsd_mod.Decoder(seed=SEED)
    yield d
    d.model.close()


@pytest.fixture(scope="module")
def donor(decoder):
    """The donor of condition (d): a decoder forward at L = 8, B = 2."""
    lat = _normal(9000, 2, 4, 8, 8)
    return lambda: decoder.forward(lat)


@pytest.fixture(scope="module")
def tiny_donor(tsd_mod, tiny):
    """... and for the decoder's own cases a Tiny UNet forward at L = 8, B = 2."""
    lat, cx = _normal(9001, 2, 4, 8, 8), _normal(9002, 2, T, 768)
    temb = np.repeat(tsd_mod.get_time_embedding(500.0).reshape(1, 320), 2, axis=0)
    return lambda: tiny.forward(lat, cx, temb)


@pytest.fixture(scope="module")
def sd15(gpu_ctx, tsd_mod):
    d = tsd_mod.Diffusion(seed=SEED, variant="diffusion_sd15")
    yield d
    d.model.close()


def _wake_zero_convs(model):
    """A seeded ControlNet keeps its zero convolutions at zero, and all its residuals with them: give them 1 / sqrt(fan_in) weights."""
    g = np.random.default_rng(5)
    for i, (name, shape, used, bound) in enumerate(model.specs):
        if used and bound == 0.0 and name.endswith(".kernel") and name.startswith(("zero.", "hint.conv8")):
            b = 1.0 / np.sqrt(float(np.prod(shape[1:])))
            model.set_param(i, g.uniform(-b, b, size=shape).astype(np.float32))


@pytest.fixture(scope="module")
def controlnet(gpu_ctx, tsd_mod):
    cn = tsd_mod.ControlNet(seed=SEED + 1)
    _wake_zero_convs(cn.model)
    yield cn
    cn.model.close()


@pytest.fixture(scope="module")
def ip(gpu_ctx, tsd_mod):
    a = tsd_mod.IPAdapter(seed=SEED + 2)
    yield a
    a.model.close()


@pytest.fixture(scope="module")
def ip_plus(gpu_ctx, tsd_mod):
    a = tsd_mod.IPAdapter(seed=SEED + 3, variant="ip_adapter_plus_sd15")
    yield a
    a.model.close()


def _temb(tsd_mod, B, t=500.0):
    return np.repeat(tsd_mod.get_time_embedding(float(t)).reshape(1, 320), B, axis=0)


# ---- 1. block-level ops: host weights, packed into the arena by the call ------------------------------------------------------------------
def _self_attention(S):
    def make(tsd):
        D, H = 320, 8
        a = tsd.Self_Attention(H, D, in_bias=False)
        a.in_proj.weight, a.out_proj.weight, a.out_proj.bias = _w(19, 3 * D, D), _w(21, D, D), randn(22, D) * 0.1
        x = randn(18, S, D)
        return lambda: a.forward(x)
    return make


def _cross_attention(S, Tk):
    def make(tsd):
        D, H, Dc = 320, 8, 768
        a = tsd.Cross_Attention(H, D, Dc, in_bias=False)
        a.q_proj.weight, a.k_proj.weight, a.v_proj.weight = _w(25, D, D), _w(26, D, Dc), _w(27, D, Dc)
        a.out_proj.weight, a.out_proj.bias = _w(28, D, D), randn(29, D) * 0.1
        x, c = randn(23, S, D), randn(24, Tk, Dc)
        return lambda: a.forward(x, c)
    return make


def _unet_attention_block(side):
    def make(tsd):
        nh, ne = 8, 40
        Cc = nh * ne
        a, P = tsd.Unet_Attention_Block(nh, ne), _attn_params("a", Cc, 70)
        a.layer2.kernel, a.layer2.bias = P["a.layer2.kernel"], P["a.layer2.bias"]
        a.layer4.in_proj.weight = P["a.layer4.in_proj.weight"]
        a.layer4.out_proj.weight, a.layer4.out_proj.bias = P["a.layer4.out_proj.weight"], P["a.layer4.out_proj.bias"]
        a.layer6.q_proj.weight, a.layer6.k_proj.weight = P["a.layer6.q_proj.weight"], P["a.layer6.k_proj.weight"]
        a.layer6.v_proj.weight = P["a.layer6.v_proj.weight"]
        a.layer6.out_proj.weight, a.layer6.out_proj.bias = P["a.layer6.out_proj.weight"], P["a.layer6.out_proj.bias"]
        a.layer8.weight, a.layer8.bias = P["a.layer8.weight"], P["a.layer8.bias"]
        a.layer9.weight, a.layer9.bias = P["a.layer9.weight"], P["a.layer9.bias"]
        a.layer10.kernel, a.layer10.bias = P["a.layer10.kernel"], P["a.layer10.bias"]
        x, c = randn(60, Cc, side, side), randn(61, T, 768)
        return lambda: a.forward(x, c)
    return make


def _vae_attention_block(Cc, side, wide=None):
    def make(tsd):
        a = tsd.Attention_Block(Cc)
        a.attention.in_proj.weight, a.attention.in_proj.bias = _w(101, 3 * Cc, Cc), randn(102, 3 * Cc) * 0.1
        a.attention.out_proj.weight, a.attention.out_proj.bias = _w(103, Cc, Cc), randn(104, Cc) * 0.1
        x = randn(100, Cc, side, wide or side)
        return lambda: a.forward(x)
    return make


def _unet_res_block(cin, cout):
    def make(tsd):
        r, P = tsd.Unet_Residual_Block(cin, cout), _res_params("r", cin, cout, 40)
        r.layer2.kernel, r.layer2.bias = P["r.layer2.kernel"], P["r.layer2.bias"]
        r.layer3.weight, r.layer3.bias = P["r.layer3.weight"], P["r.layer3.bias"]
        r.layer5.kernel, r.layer5.bias = P["r.layer5.kernel"], P["r.layer5.bias"]
        r.layer6.kernel, r.layer6.bias = P["r.layer6.kernel"], P["r.layer6.bias"]
        x, time = randn(30, cin, 8, 8), randn(31, 1, 1280)
        return lambda: r.forward(x, time)
    return make


def _vae_res_block(cin, cout):
    def make(tsd):
        r = tsd.Res_Block(cin, cout)
        r.conv1.kernel, r.conv1.bias = _w(91, cout, cin, 3, 3), randn(92, cout) * 0.1
        r.conv2.kernel, r.conv2.bias = _w(93, cout, cout, 3, 3), randn(94, cout) * 0.1
        r.res_conv_layer.kernel, r.res_conv_layer.bias = _w(95, cout, cin, 1, 1), randn(96, cout) * 0.1
        x = randn(90, cin, 8, 8)
        return lambda: r.forward(x)
    return make


def _conv2d(cin):
    def make(tsd):
        c = tsd.Conv2D(cin, 64, 3, (1, 1), (1, 1))
        c.kernel, c.bias = _w(2, 64, cin, 3, 3), randn(3, 64) * 0.1
        x = randn(1, cin, 8, 8)
        return lambda: c.forward(x)
    return make


def _linear(M, K):
    def make(tsd):
        l = tsd.Linear(K, 96)
        l.weight, l.bias = _w(12, 96, K), randn(13, 96) * 0.1
        x = randn(11, M, K)
        return lambda: l.forward(x)
    return make


def _matmul(M, K):
    def make(tsd):
        a, b = randn(14, 2, M, K), randn(15, 2, K, 24)
        return lambda: tsd.matmul(a, b)
    return make


def _time_embedding_mlp(tsd):
    from oracle import ops
    t = tsd.Time_Embedding(320)
    t.layer1.weight, t.layer1.bias, t.layer2.weight, t.layer2.bias = _w(110, 1280, 320), randn(111, 1280) * 0.1, _w(112, 1280, 1280), randn(113, 1280) * 0.1
    e = ops.time_embedding(500.0)
    return lambda: t.forward(e)


def _upsample(tsd):
    x = randn(9, 6, 5, 7)
    return lambda: tsd.Upsample(2).forward(x)


def _groupnorm(tsd):
    x = randn(5, 64, 3, 5) * 2.0 + 0.5
    return lambda: tsd.GroupNorm(32, 64).forward(x)


def _layernorm(tsd):
    x = randn(6, 3, 320) * 3.0 + 1.0
    return lambda: tsd.LayerNorm(320).forward(x)


BLOCK_OPS = {
    # the stand-alone self-attention and the VAE block refuse a key count that is no multiple of 8 (test_entries_without_a_key_pad...):
    # their second shape is the smallest odd one they accept, a partial query / key tile without a pad column
    "self_attention_S64": _self_attention(64), "self_attention_S24": _self_attention(24),
    "cross_attention_S64_T77": _cross_attention(64, 77), "cross_attention_S20_T5": _cross_attention(20, 5),
    "cross_attention_S64_T5": _cross_attention(64, 5), "cross_attention_S20_T77": _cross_attention(20, 77),
    "unet_attention_block_S64": _unet_attention_block(8),     # the fused head / tail kernels
    "unet_attention_block_S36": _unet_attention_block(6),     # Sp = 40 != S: the op-by-op path and its memset of V^T
    # one head of width C: C = 128 runs GEMM - softmax - GEMM (S % 64 == 0 only), C = 64 the flash core
    "vae_attention_block_C128_S64": _vae_attention_block(128, 8), "vae_attention_block_C64_S40": _vae_attention_block(64, 5, 8),
    "unet_residual_block_64_64": _unet_res_block(64, 64), "unet_residual_block_64_128": _unet_res_block(64, 128),
    "vae_res_block_64_64": _vae_res_block(64, 64), "vae_res_block_64_128": _vae_res_block(64, 128),
    "conv2d_cin4": _conv2d(4), "conv2d_cin64": _conv2d(64),   # Cin = 4: the channel pad to 64
    "linear_M1_K77": _linear(1, 77), "linear_M65_K77": _linear(65, 77), "linear_M1_K128": _linear(1, 128), "linear_M65_K128": _linear(65, 128),
    "matmul_M1_K77": _matmul(1, 77), "matmul_M65_K77": _matmul(65, 77), "matmul_M1_K128": _matmul(1, 128), "matmul_M65_K128": _matmul(65, 128),
    "time_embedding_mlp": _time_embedding_mlp, "upsample_nearest2x": _upsample, "groupnorm": _groupnorm, "layernorm": _layernorm,
}


@pytest.mark.parametrize("name", list(BLOCK_OPS))
def test_block_op_does_not_read_the_workspace(gpu_ctx, tsd_mod, donor, name):
    hold(tsd_mod, gpu_ctx, donor, BLOCK_OPS[name](tsd_mod), name)


def test_entries_without_a_key_pad_refuse_the_shapes_that_would_need_one(gpu_ctx, tsd_mod):
    """tsd_self_attention_f32 at S = 20 (Sp = 24) and tsd_vae_attention_block_f32 at S = 36 (Sp = 40) would read V^T pad columns nobody
    writes: both entries refuse S % 8 != 0 with TSD_E_SHAPE instead, so there is no such path to hold (tsd_unet_attention_block_f32 at
    S = 36 is the entry that has one)."""
    for make in (_self_attention(20), _vae_attention_block(64, 6)):
        with pytest.raises(tsd_mod.TsdError) as e:
            make(tsd_mod)()
        assert e.value.code == tsd_mod._lib.TSD_E_SHAPE


# ---- 2. model forwards -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 2))
def test_tiny_unet_forward(gpu_ctx, tsd_mod, donor, tiny, B):
    lat, cx, temb = _normal(100, B, 4, 8, 8), _normal(101, B, T, 768), _temb(tsd_mod, B)
    hold(tsd_mod, gpu_ctx, donor, lambda: tiny.forward(lat, cx, temb), f"Tiny UNet forward, B = {B}")


@pytest.mark.parametrize("switch", ("fused_attention", "qkv_fuse", "res_fuse_skip", "ups_fold"))
def test_tiny_unet_forward_with_a_graph_option_off(gpu_ctx, tsd_mod, donor, tiny, switch):
    lat, cx, temb = _normal(100, 2, 4, 8, 8), _normal(101, 2, T, 768), _temb(tsd_mod, 2)
    with option(tsd_mod, gpu_ctx, switch, 0):
        hold(tsd_mod, gpu_ctx, donor, lambda: tiny.forward(lat, cx, temb), f"Tiny UNet forward, {switch} off")


@pytest.mark.parametrize("LH,LW", ((16, 16), (16, 32)), ids=("16x16", "16x32"))
def test_sd15_forward(gpu_ctx, tsd_mod, donor, sd15, LH, LW):
    lat, cx, temb = _normal(110, 2, 4, LH, LW), _normal(111, 2, T, 768), _temb(tsd_mod, 2)
    hold(tsd_mod, gpu_ctx, donor, lambda: sd15.forward(lat, cx, temb), f"diffusion_sd15 forward, {LH}x{LW}")


def test_sd2_forward(gpu_ctx, tsd_mod, donor):
    d = tsd_mod.Diffusion(seed=SEED + 4, variant="diffusion_sd2")
    try:
        lat, cx, temb = _normal(120, 2, 4, 16, 16), _normal(121, 2, T, 1024), _temb(tsd_mod, 2)
        hold(tsd_mod, gpu_ctx, donor, lambda: d.forward(lat, cx, temb), "diffusion_sd2 forward, 16x16")
    finally:
        d.model.close()


def _control_inputs(B=2, L=16):
    return _normal(130, B, 4, L, L), _normal(131, B, T, 768), 127.5 + 60.0 * _normal(132, B, 3, 8 * L, 8 * L)


def test_controlnet_forward(gpu_ctx, tsd_mod, donor, controlnet):
    lat, cx, hint = _control_inputs()
    temb = _temb(tsd_mod, 2)
    res = controlnet.forward(lat, cx, temb, hint)
    assert any(r.any() for r in res), "the residuals are all zero: the test would hold nothing"
    hold(tsd_mod, gpu_ctx, donor, lambda: controlnet.forward(lat, cx, temb, hint), "tsd_controlnet_forward_hw")


@pytest.mark.parametrize("stats", (1, 0))
def test_controlled_forward(gpu_ctx, tsd_mod, donor, sd15, controlnet, stats):
    lat, cx, hint = _control_inputs()
    temb, scale = _temb(tsd_mod, 2), np.array([1.0, 0.5], np.float32)
    with option(tsd_mod, gpu_ctx, "control_stats", stats):
        hold(tsd_mod, gpu_ctx, donor, lambda: sd15.forward(lat, cx, temb, control=controlnet, hint=hint, control_scale=scale),
             f"controlled forward, control_stats = {stats}")


@pytest.mark.parametrize("N", (1, 4, 16))
def test_adapted_forward(gpu_ctx, tsd_mod, donor, sd15, ip, N):
    lat, cx, temb = _normal(140, 2, 4, 16, 16), _normal(141, 2, T, 768), _temb(tsd_mod, 2)
    tok, scale = _normal(142 + N, 2, N, 768), np.array([1.0, 0.6], np.float32)
    hold(tsd_mod, gpu_ctx, donor, lambda: sd15.forward(lat, cx, temb, ip_adapter=ip, ip_tokens=tok, ip_scale=scale), f"adapted forward, N = {N}")


def test_ip_adapter_project(gpu_ctx, tsd_mod, donor, ip):
    emb = _normal(150, 2, 1024)
    hold(tsd_mod, gpu_ctx, donor, lambda: ip.project(emb), "tsd_ip_adapter_project")


@pytest.mark.parametrize("S", (5, 257))
def test_ip_adapter_resample(gpu_ctx, tsd_mod, donor, ip_plus, S):
    hid = _normal(151 + S, 2, S, 1280)
    hold(tsd_mod, gpu_ctx, donor, lambda: ip_plus.resample(hid), f"tsd_ip_adapter_resample, S = {S}")


@pytest.mark.parametrize("variant", ("clip", "clip_sd2"))
def test_clip_text_forward(gpu_ctx, tsd_mod, donor, variant):
    m = tsd_mod.CLIP(seed=SEED + 5, variant=variant)
    try:
        tokens = np.random.default_rng(6).integers(0, 49408, size=(2, T)).astype(np.int32)
        hold(tsd_mod, gpu_ctx, donor, lambda: m.forward(tokens), f"tsd_clip_forward, {variant}")
    finally:
        m.model.close()


@pytest.fixture(scope="module")
def vision(gpu_ctx, tsd_mod):
    m = tsd_mod.CLIPVision(seed=SEED + 6)
    yield m
    m.model.close()


@pytest.mark.parametrize("H,W", ((224, 224), (64, 96)), ids=("224x224", "64x96"))
def test_clip_vision_forward(gpu_ctx, tsd_mod, donor, vision, H, W):
    images = np.clip(127.5 + 60.0 * _normal(160 + H, 2, 3, H, W), 0.0, 255.0)
    hold(tsd_mod, gpu_ctx, donor, lambda: vision.forward(images, hidden=True), f"tsd_clip_vision_forward, {H}x{W}")


def test_encoder_forward(gpu_ctx, tsd_mod, donor):
    e = tsd_mod.Encoder(seed=SEED + 7)
    try:
        img, nz = _normal(170, 2, 3, 64, 64), _normal(171, 2, 4, 8, 8)
        hold(tsd_mod, gpu_ctx, donor, lambda: e.forward(img, nz), "encoder forward, L = 8")
    finally:
        e.model.close()


def test_decoder_forward(gpu_ctx, tsd_mod, tiny_donor, decoder):
    lat = _normal(172, 2, 4, 8, 8)
    hold(tsd_mod, gpu_ctx, tiny_donor, lambda: decoder.forward(lat), "decoder forward, L = 8")


def test_lora_merge_op(gpu_ctx, tsd_mod, donor):
    from tsd._lib import check, ptr
    O, I, r = 37, 77, 4      # I = 77: the K pad of the packed weight
    w, up, down = _normal(180, O, I), 0.1 * _normal(181, O, r), 0.1 * _normal(182, r, I)

    def merge():
        out = np.empty((O, I), np.float32)
        check(tsd_mod._lib.lib().tsd_lora_merge_f32(gpu_ctx.h, ptr(w), O, I, 0, 0, 0, O, ptr(up), ptr(down), r, 0.5, ptr(out)))
        return out
    hold(tsd_mod, gpu_ctx, donor, merge, "tsd_lora_merge_f32")


def test_model_lora_add_and_clear(gpu_ctx, tsd_mod, donor, tiny):
    name = "unet.layer3.layer6.k_proj.weight"
    m = tiny.model
    rows, cols = m.specs[m.param_index(name)][1]
    up, down = 0.1 * _normal(183, rows, 4), 0.1 * _normal(184, 4, cols)
    base = m.get_param(name)

    def add_and_clear():
        try:
            m.lora_add(name, up, down, 0.5)
            merged = m.get_param(name)
        finally:
            m.lora_clear()
        return merged, m.get_param(name)
    hold(tsd_mod, gpu_ctx, donor, add_and_clear, "tsd_model_lora_add / lora_clear")
    merged, cleared = add_and_clear()
    assert np.array_equal(_bits(cleared), _bits(base)) and not np.array_equal(merged, base)


# ---- 3. sessions: a scribble before every call --------------------------------------------------------------------------------------------
N_TRAIN, STEPS = 1000, 3
B, L = 2, 8
SESSION_CASES = [("epsilon", False, ("ddpm", 0.0, "leading")), ("epsilon", False, ("ddim", 0.5, "trailing")),
                 ("epsilon", False, ("dpmpp_2m", 0.0, "trailing")),
                 ("v", True, ("ddpm", 0.0, "trailing")), ("v", True, ("ddim", 0.5, "trailing")), ("v", True, ("dpmpp_2m", 0.0, "trailing"))]
SESSION_IDS = [f"{p}-{s[0]}" for p, _, s in SESSION_CASES]


def _mask(k, LH=L, LW=L):
    cell = np.arange(LH * LW).reshape(LH, LW)
    v = (cell * (2 * k + 3) + k) % 13
    return np.where(v < 4, 0.0, np.where(v > 9, 1.0, v / 16.0)).astype(np.float32)


def _configure(s, pred, ztsnr, sampler, steps=STEPS):
    s.set_prediction(pred, ztsnr)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, steps, 0)


def _lockstep(tsd_mod, unet, dec, before, pred, ztsnr, sampler, uploaded_noise=False):
    """Every feature of a lockstep session on a Tiny UNet, `before()` ahead of every call: -> (latents, images)."""
    lat, cx, ucx = _normal(200, B, 4, L, L), _normal(201, B, T, 768), _normal(202, B, T, 768)
    masks, known = np.stack([_mask(0), _mask(1)]), _normal(203, B, 4, L, L)
    s = tsd_mod.Session(unet.model, dec.model, B, L, T, cfg=True)
    try:
        _configure(s, pred, ztsnr, sampler)
        if uploaded_noise:
            before(); s.upload(lat, cx, ucx, _normal(204, STEPS, B, 4, L, L), cfg_scale=5.0)
            before(); s.set_inpaint(masks, known, _normal(205, B, 4, L, L))
        else:
            before(); s.upload(lat, cx, ucx, None, cfg_scale=5.0)
            before(); s.set_seeds([91, 92])
            before(); s.seed_latents()
            before(); s.set_inpaint(masks, known, seeded=True)
        before(); s.set_guidance_rescale(0.7)
        for i in range(STEPS):
            before(); s.step(i)
        before(); s.decode()
        before(); out = s.latents()
        before(); img = s.images(rescale=True)
        return out, img
    finally:
        s.close()


@pytest.mark.parametrize("hoist", (1, 0), ids=("hoist", "nohoist"))
@pytest.mark.parametrize("pred,ztsnr,sampler", SESSION_CASES, ids=SESSION_IDS)
def test_lockstep_session_scribbled_between_calls(gpu_ctx, tsd_mod, tiny, decoder, pred, ztsnr, sampler, hoist):
    what = f"lockstep session, {pred}, {sampler[0]}, hoist {hoist}"
    with option(tsd_mod, gpu_ctx, "session_hoist", hoist):
        _lockstep(tsd_mod, tiny, decoder, lambda: None, pred, ztsnr, sampler)   # sizes the arena and the staging buffer
        results = [(f"scribble 0x{byte:02X} before every call", list(_lockstep(tsd_mod, tiny, decoder, lambda b=byte: gpu_ctx.scribble(b), pred, ztsnr, sampler)))
                   for byte in (0x00, 0xFF)]
    compare(results, what)


def _slot_request(k):
    return dict(ctx=_normal(300 + 10 * k, T, 768), uctx=_normal(301 + 10 * k, T, 768), seed=3000017 * (k + 1) + 31, scale=(7.5, 3.0, 5.0)[k],
                phi=(0.7, 0.3, 0.0)[k], mask=_mask(k), known=_normal(302 + 10 * k, 4, L, L), lat=_normal(303 + 10 * k, 4, L, L))


def _slots(tsd_mod, unet, before, pred, ztsnr, sampler):
    """Slot 0 runs a seeded inpainting request over all steps; slot 1 an img2img request from index 1, and is refilled when it is done
    while slot 0 is mid-flight.  `before()` ahead of every call: -> the three requests' latents."""
    reqs = [_slot_request(k) for k in range(3)]
    s = tsd_mod.Session(unet.model, None, B, L, T, cfg=True)
    try:
        _configure(s, pred, ztsnr, sampler)
        before(); s.slots_open()
        r = reqs[0]
        before(); s.slot_start(0, r["ctx"], r["uctx"], seed=r["seed"], cfg_scale=r["scale"])
        before(); s.slot_set_inpaint(0, r["mask"], r["known"])
        before(); s.slot_set_guidance_rescale(0, r["phi"])
        r = reqs[1]
        before(); s.slot_start(1, r["ctx"], r["uctx"], latents=r["lat"], noise_at_start=True, seed=r["seed"], start_index=1, cfg_scale=r["scale"])
        before(); s.slot_set_guidance_rescale(1, r["phi"])
        got, which = {}, {0: 0, 1: 1}
        for tick in range(STEPS + 1):
            before(); done = s.advance()
            for b in done:
                before(); got[which[b]] = s.slot_latents(b)
            if tick == 1:
                assert done == [1], done
                r = reqs[2]
                before(); s.slot_start(1, r["ctx"], r["uctx"], latents=r["lat"], noise_at_start=True, seed=r["seed"], start_index=1, cfg_scale=r["scale"])
                which[1] = 2
        assert sorted(got) == [0, 1, 2] and s.slots_active() == 0, sorted(got)
        return [got[k] for k in range(3)]
    finally:
        s.close()


@pytest.mark.parametrize("hoist", (1, 0), ids=("hoist", "nohoist"))
@pytest.mark.parametrize("pred,ztsnr,sampler", [SESSION_CASES[0], SESSION_CASES[5]], ids=[SESSION_IDS[0], SESSION_IDS[5]])
def test_slot_session_scribbled_between_calls(gpu_ctx, tsd_mod, tiny, pred, ztsnr, sampler, hoist):
    with option(tsd_mod, gpu_ctx, "session_hoist", hoist):
        _slots(tsd_mod, tiny, lambda: None, pred, ztsnr, sampler)
        results = [(f"scribble 0x{byte:02X} before every call", _slots(tsd_mod, tiny, lambda b=byte: gpu_ctx.scribble(b), pred, ztsnr, sampler))
                   for byte in (0x00, 0xFF)]
    compare(results, f"slot session, {pred}, {sampler[0]}, hoist {hoist}")


def test_sd15_session_with_control_and_ip_adapter_scribbled_between_calls(gpu_ctx, tsd_mod, sd15, controlnet, ip):
    """The full-size case: the ControlNet's residuals and the adapter's K_ip / V_ip^T cross from one call of the session to the next."""
    LL, steps = 16, 2
    lat, cx, ucx = _normal(400, B, 4, LL, LL), _normal(401, B, T, 768), _normal(402, B, T, 768)
    hint = 127.5 + 60.0 * _normal(403, B, 3, 8 * LL, 8 * LL)
    tok, utok = ip.project(_normal(404, B, 1024)), ip.project(np.zeros((B, 1024), np.float32))

    def run(before):
        s = tsd_mod.Session(sd15.model, None, B, LL, T, cfg=True)
        try:
            _configure(s, "epsilon", False, ("ddim", 0.0, "leading"), steps)
            before(); s.upload(lat, cx, ucx, None, cfg_scale=5.0)
            before(); s.set_control(controlnet, hint, scale=0.8)
            before(); s.set_ip_adapter(ip, tok, utok, scale=0.7)
            assert s.control_active and s.ip_adapter_active
            for i in range(steps):
                before(); s.step(i)
            before()
            return [s.latents()]
        finally:
            s.close()
    run(lambda: None)
    compare([(f"scribble 0x{byte:02X} before every call", run(lambda b=byte: gpu_ctx.scribble(b))) for byte in (0x00, 0xFF)],
            "diffusion_sd15 session with set_control and set_ip_adapter")


# ---- 4. fresh session memory: TSD_DEBUG_POISON, bits 8 (the buffers a session grows) and 16 (staging) included --------------------------------
def test_fresh_allocations_poisoned_with_two_bytes_give_the_same_bits(gpu_ctx, tsd_mod, monkeypatch):
    """Two contexts created under TSD_DEBUG_POISON = 0x00 and 0xFF (TSD_DEBUG_POISON_WHAT at its default, 31), a Tiny UNet and a decoder on
    each: a lockstep session with every feature on (seeded, and with an uploaded noise tensor and the hoist's tables) and a slot session.
    Nothing is warmed up: every arena, staging buffer, session state block and session buffer is read as allocated."""
    results = []
    case = SESSION_CASES[1]   # DDIM with eta > 0: every step adds noise
    for byte in (0x00, 0xFF):
        c = replay.ctx_with(tsd_mod, gpu_ctx, monkeypatch, "TSD_DEBUG_POISON", byte)
        unet, dec = tsd_mod.Diffusion(seed=SEED, ctx=c), tsd_mod.Decoder(seed=SEED, ctx=c)
        try:
            out = list(_lockstep(tsd_mod, unet, dec, lambda: None, *case))
            out += list(_lockstep(tsd_mod, unet, dec, lambda: None, *case, uploaded_noise=True))
            out += _slots(tsd_mod, unet, lambda: None, *case)
            results.append((f"TSD_DEBUG_POISON = 0x{byte:02X}", out))
        finally:
            unet.model.close(); dec.model.close(); c.close()
    compare(results, "sessions on freshly poisoned contexts")


def test_scribble_refuses_bad_arguments_and_leaves_the_flags_alone(gpu_ctx, tsd_mod):
    lib = tsd_mod._lib.lib()
    E = tsd_mod._lib
    assert lib.tsd_debug_scribble(None, 0) == E.TSD_E_ARG
    for byte in (-1, 256):
        assert lib.tsd_debug_scribble(gpu_ctx.h, byte) == E.TSD_E_ARG, byte
    lib.tsd_debug_nonfinite_count(gpu_ctx.h, 1)
    errs = lib.tsd_debug_splitk_errors(gpu_ctx.h)
    gpu_ctx.scribble(0xFF)
    gpu_ctx.synchronize()                                       # status words and hand-off flags are not scribbled: nothing to report
    assert lib.tsd_debug_nonfinite_count(gpu_ctx.h, 0) == 0 and lib.tsd_debug_splitk_errors(gpu_ctx.h) == errs
