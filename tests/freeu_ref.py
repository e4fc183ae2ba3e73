"""Float64 restatement of FreeU (Si et al. 2023) and the error bound the device launch is held to.

TEST INFRASTRUCTURE.  Five things:

  * `fourier_filter_fft`: the literal restatement of diffusers' `fourier_filter(x, threshold=1, scale=s)` - fftn, fftshift, the 2 x 2 mask
    around the centre, ifftshift, ifftn, `.real` - the definition.
  * `fourier_filter_closed`: x + (s - 1) P(x) from seven real sums per plane, the form the kernel evaluates (csrc/kernels_freeu.hip).
    tests/test_freeu_cpu.py holds the two to each other at 1e-12.
  * `hidden_constant` / `hidden_modulated`: the two ways the backbone half is scaled.
  * `skip_bound` / `hidden_bound`: element-wise bounds for |device - float64| of the launch on fp16 inputs, derived below.
  * `unet_full_freeu` / `diffusion_freeu`: oracle.models' full-size loop with the two rewrites at the pop steps (the skip through the FFT
    restatement, not the closed form), an optional list of ControlNet residuals, and the four near misses of an implementation.

The bounds.  u = 2^-24 (fp32 unit roundoff).  halfulp16(v) = max(2^-25, 2^(floor(log2 |v|) - 11)): half a unit in the last place of fp16
at magnitude v (2^-25: half the subnormal spacing).  A device value that is the fp16 rounding of an fp32 value within e of the exact y lies
within e + halfulp16(|y| + e) of y.

Skip.  Inputs r are fp16 (exact in fp32).  Per plane of n = H W pixels let A = sum |r|.
  (1) coefficients: a table entry is the correctly rounded fp32 of |t| <= 1: error <= u.  cxy, sxy are one product, one fma of such
      entries: error <= 2u (operands) + 2u (two roundings) + second order.  Every coefficient c_k the device uses: |c~_k - c_k| <= 5u.
  (2) sums: S~_k is an fp32 sum of n terms fma'd in some fixed order (pixel lanes, then the lane totals): any order satisfies
      |S~_k - sum r c~_k| <= gamma_n sum |r c~_k|, gamma_n = n u / (1 - n u) <= 1.01 n u for n <= 2^16.  With (1):
      |S~_k - S_k| <= e_S := (1.01 n + 5) u A      (|c~_k| <= 1 + 5u is absorbed by the 1.01).
  (3) N = S_0 + sum_{k=1..6} S_k c_k by six fmas: sum_k (e_S |c~_k| + |S_k| 5u) + gamma_7 sum_k |S_k c_k| <= 7 e_S + 35 u A + 8 u 7 A
      (|S_k| <= A): |N~ - N| <= e_N := 7 e_S + 91 u A, and |N| <= 7 A.
  (4) y = r + g N, g = (s - 1) / n rounded once to fp32 (relative error u), one fma: the fp32 value before the fp16 rounding is within
      e = |g| e_N + u |g| 7 A + u (|y| + |g| e_N) <= |s - 1| / n * A u (7 (1.01 n + 5) + 99) + 2 u |y|    of y.
  bound = e + halfulp16(|y| + e).

Hidden, constant.  y = b h with b an fp32 and h an fp16: one fp32 product, e = u |y|; bound = e + halfulp16(|y| + e).

Hidden, modulated.  Per pixel p let Ah[p] = sum_c |h[p][c]|.
  (5) mean: fp32 sum of Ch terms in a fixed order, then one division by Ch: |m~[p] - m[p]| <= e_m[p] := 1.01 u Ah[p] + u |m[p]|
      (gamma_Ch Ah / Ch + the division's rounding).  E := max_p e_m[p].
  (6) lo~ / hi~ are the exact minimum / maximum of the m~: each within E of lo / hi.  d~ = fl(hi~ - lo~): |d~ - d| <= e_d := 2E + u (d + 2E).
  (7) n~ = fl(fl(m~ - lo~) / d~): the numerator is within e_m[p] + E + u d <= 2E + u d of m - lo, and with 0 <= n <= 1
      |n~ - n| <= dn := (2E + u d + e_d) / (d - e_d) + 2u          - the 1 / (hi - lo) amplification of the mean's error.
      Where d <= 2 e_d (the normalisation is ill-conditioned; hi == lo included) dn := 1: both sides have n in [0, 1].
  (8) f = fma(fl(b - 1), n~, 1): |f~ - f| <= |b - 1| (dn + u) + u (|f| + |b - 1| dn); y = f h, one fp32 product:
      e = |h| (|b - 1| (dn + u) + u (|f| + |b - 1| dn)) + u (|y| + |h| |b - 1| dn); bound = e + halfulp16(|y| + e).
  Where every pixel of a sample holds the same channel vector, m~ is the same fp32 at every pixel, so d~ = 0 and n~ = 0 exactly: the device
  returns h bit for bit (the hi == lo rule), which the test asserts directly instead of using dn = 1.
"""
import numpy as np

from oracle import models, ops
from oracle.models import _conv, time_embedding_mlp, unet_attention_block, unet_residual_block
from oracle.ops import DEFAULT
from oracle.spec import FULL_UNET_STEPS

U = 2.0 ** -24
CONSTANT, MODULATED = 0, 1
# 1-based layer numbers of the decoder residual blocks, in pop order
POP_LAYERS = [i for i, (k, _, f) in enumerate(FULL_UNET_STEPS, start=1) if f == "pop"]
assert [i - 1 for i in POP_LAYERS] == [21, 22, 23, 25, 27, 29, 32, 34, 36, 39, 41, 43]
assert all(FULL_UNET_STEPS[i - 1][0] == "res" for i in POP_LAYERS)
NEAR_MISSES = ("upper_half", "filter_hidden", "s_minus_1")


def hidden_widths():
    """Ch of the twelve pop steps, read from the step table: the input width of the block minus its skip's width."""
    widths, out, c = [], [], 0
    for kind, a, flags in FULL_UNET_STEPS:
        if flags == "pop":
            out.append(a[0] - widths.pop())
        c = a[1] if kind in ("conv", "upconv", "res") else c
        if flags == "push":
            widths.append(c)
    return out


# ---- the skip filter ---------------------------------------------------------------------------------------------------------------------
def fourier_filter_fft(x, s, threshold=1):
    """x (..., H, W) real -> the planes with the centre 2 x 2 bins of the shifted spectrum scaled by s, float64."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    f = np.fft.fftshift(np.fft.fftn(x, axes=(-2, -1)), axes=(-2, -1))
    mask = np.ones(x.shape, np.float64)
    cr, cc = H // 2, W // 2
    mask[..., cr - threshold:cr + threshold, cc - threshold:cc + threshold] = s
    return np.fft.ifftn(np.fft.ifftshift(f * mask, axes=(-2, -1)), axes=(-2, -1)).real


def _basis(H, W):
    y, x = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    cy, sy = np.cos(2 * np.pi * y / H)[:, None], np.sin(2 * np.pi * y / H)[:, None]
    cx, sx = np.cos(2 * np.pi * x / W)[None, :], np.sin(2 * np.pi * x / W)[None, :]
    one = np.ones((H, W))
    return [one, cy * one, sy * one, cx * one, sx * one, cy * cx - sy * sx, sy * cx + cy * sx]


def projection_closed(x):
    """P(x) of the docstring: (..., H, W) float64."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    P = np.zeros_like(x)
    for c in _basis(H, W):
        P += (x * c).sum((-2, -1), keepdims=True) * c
    return P / (H * W)


def fourier_filter_closed(x, s):
    x = np.asarray(x, np.float64)
    return x + (float(s) - 1.0) * projection_closed(x)


# ---- the hidden half ---------------------------------------------------------------------------------------------------------------------
def modulation(h):
    """h (B, H, W, C) -> n (B, H, W, 1): the channel mean, min-max normalised per sample; 0 where hi == lo."""
    h = np.asarray(h, np.float64)
    m = h.mean(-1, keepdims=True)
    lo, hi = m.min((1, 2), keepdims=True), m.max((1, 2), keepdims=True)
    d = hi - lo
    return np.where(d > 0, (m - lo) / np.where(d > 0, d, 1.0), 0.0)


def hidden_constant(h, b):
    h = np.asarray(h, np.float64).copy()
    h[..., : h.shape[-1] // 2] *= float(b)
    return h


def hidden_modulated(h, b):
    h = np.asarray(h, np.float64).copy()
    h[..., : h.shape[-1] // 2] *= (float(b) - 1.0) * modulation(h) + 1.0
    return h


# ---- the bounds --------------------------------------------------------------------------------------------------------------------------
def halfulp16(v):
    v = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -24)))
    return np.maximum(2.0 ** -25, 2.0 ** (e - 11))


def skip_bound(r, s):
    """r fp16 (B, H, W, C), NHWC -> (exact float64 result, element-wise bound), the planes being (H, W) of every (b, c)."""
    r64 = np.moveaxis(np.asarray(r, np.float64), -1, 1)          # (B, C, H, W)
    n = r64.shape[-1] * r64.shape[-2]
    y = fourier_filter_closed(r64, s)
    A = np.abs(r64).sum((-2, -1), keepdims=True)
    e = abs(float(s) - 1.0) / n * A * U * (7 * (1.01 * n + 5) + 99) + 2 * U * np.abs(y)
    return np.moveaxis(y, 1, -1), np.moveaxis(e + halfulp16(np.abs(y) + e), 1, -1)


def hidden_bound(h, b, mode):
    """h fp16 (B, H, W, C) -> (exact float64 result, element-wise bound); the upper half of the channels has bound 0."""
    h64 = np.asarray(h, np.float64)
    half = h64.shape[-1] // 2
    bound = np.zeros_like(h64)
    if mode == CONSTANT:
        y = hidden_constant(h64, b)
        e = U * np.abs(y[..., :half])
        bound[..., :half] = e + halfulp16(np.abs(y[..., :half]) + e)
        return y, bound
    y = hidden_modulated(h64, b)
    m = h64.mean(-1, keepdims=True)
    e_m = 1.01 * U * np.abs(h64).sum(-1, keepdims=True) + U * np.abs(m)
    E = e_m.max((1, 2), keepdims=True)
    d = m.max((1, 2), keepdims=True) - m.min((1, 2), keepdims=True)
    e_d = 2 * E + U * (d + 2 * E)
    ok = d > 2 * e_d
    dn = np.where(ok, (2 * E + U * d + e_d) / np.where(ok, d - e_d, 1.0) + 2 * U, 1.0)
    b1 = abs(float(b) - 1.0)
    f = (float(b) - 1.0) * modulation(h64) + 1.0
    ah = np.abs(h64[..., :half])
    e = ah * (b1 * (dn + U) + U * (np.abs(f) + b1 * dn)) + U * (np.abs(y[..., :half]) + ah * b1 * dn)
    bound[..., :half] = e + halfulp16(np.abs(y[..., :half]) + e)
    return y, bound


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def freeu_pair(h, r, b, s, mode, miss=None):
    """One decoder concat's two inputs, CHW float32 -> (h', r').  miss: one of NEAR_MISSES, what a wrong implementation would do."""
    b, s = float(b), float(s)
    hh = np.moveaxis(np.asarray(h, np.float64), 0, -1)[None]    # (1, H, W, C)
    if b != 1.0:
        flip = miss == "upper_half"   # the scaled half is the upper channels: the lower half of the reversed channel axis
        src = hh[..., ::-1] if flip else hh
        out = hidden_modulated(src, b) if mode == MODULATED else hidden_constant(src, b)
        hh = out[..., ::-1] if flip else out
    h2 = np.moveaxis(hh[0], -1, 0)
    r2 = np.asarray(r, np.float64)
    if s != 1.0:
        if miss == "filter_hidden":   # the filter lands on the hidden tensor
            h2 = fourier_filter_fft(h2, s)
        elif miss == "s_minus_1":     # the bins are scaled by s - 1
            r2 = fourier_filter_fft(r2, s - 1.0)
        else:
            r2 = fourier_filter_fft(r2, s)
    return h2.astype(np.float32), r2.astype(np.float32)


def _layer(P, i, steps, h, context, time, sem, tn):
    kind, a, _ = steps[i - 1]
    name = f"unet.layer{i}"
    if kind == "conv":
        return _conv(P, name, h, (1, 1), stride=(a[3], a[3]))
    if kind == "upconv":
        return _conv(P, name, ops.upsample_nearest2x(h), (1, 1))
    if kind == "res":
        return unet_residual_block(P, name, h, time, *a, tn=tn)
    return unet_attention_block(P, name, h, context, *a, sem=sem, tn=tn)


def unet_full_freeu(P, x, context, time, table, mode=CONSTANT, steps=FULL_UNET_STEPS, sem=DEFAULT, tn=False, res=None, res_scale=0.0,
                    miss=None):
    """oracle.models.unet_full with FreeU at the pop steps: table = (b[12], s[12]) or None (the plain forward).  res: the 13 residuals of
    a ControlNet (tests/controlnet_ref.py), added scaled by res_scale BEFORE FreeU, as diffusers does.  steps: the step table
    (tests/sd2_ref.SD2_STEPS for kind 16)."""
    skips, pops = [], 0
    h = x
    rs = np.float32(res_scale)
    enc_n = POP_LAYERS[0] - 1
    for i, (_, _, flags) in enumerate(steps, start=1):
        if flags == "pop":
            k = len(skips) - 1
            r = skips.pop()
            if res is not None:
                r = r + rs * res[k]
            if table is not None:
                h, r = freeu_pair(h, r, table[0][pops], table[1][pops], mode, miss)
            pops += 1
            h = ops.concat_channels(h, r)
        h = _layer(P, i, steps, h, context, time, sem, tn)
        if i == enc_n and res is not None:
            h = h + rs * res[12]
        if flags == "push":
            skips.append(h)
    assert not skips and pops == 12
    return h


def diffusion_freeu(P, x, context, t320, table, mode=CONSTANT, steps=FULL_UNET_STEPS, tn=False, res=None, res_scale=0.0, miss=None):
    """The whole forward of one sample: x (4, LH, LW), context (T, W), t320 (320,) -> (4, LH, LW)."""
    time = time_embedding_mlp(P, t320)
    h = unet_full_freeu(P, x, context, time, table, mode, steps=steps, tn=tn, res=res, res_scale=res_scale, miss=miss)
    if tn:
        h = ops.silu(ops.group_norm_torch(h, 32, 1e-5, P["final.layer1.weight"], P["final.layer1.bias"]))
        return _conv(P, "final.layer2", h, (1, 1))
    return models.unet_output_layer(P, h)


# ---- the draw the model-level tests share -------------------------------------------------------------------------------------------------
# Chosen on the CPU (tests/test_freeu_cpu.py repeats the check for kind 6 at 16 x 16): with these parameters and FreeU values every case
# differs from the plain forward, and every near miss from the true reference, by more than 10 TOL_MODEL.  The paper's SD-1.x values
# (1.5, 1.6, 0.9, 0.2) act too weakly on these random weights for that (0.06 .. 0.1), so the test values are stronger.
MODEL_SEED = 21
MODEL_VALUES = dict(b1=2.0, b2=2.2, s1=0.5, s2=0.1)
MODEL_SHAPES = ((16, 16), (16, 32))
MODEL_KINDS = {"diffusion_sd15_torch": 768, "diffusion_sd2": 1024}   # kind -> context width
MODEL_T = 77


def model_steps(kind):
    if kind == "diffusion_sd2":
        import sd2_ref
        return sd2_ref.SD2_STEPS
    return FULL_UNET_STEPS


def model_inputs(kind, LH, LW):
    """One sample: latents (1, 4, LH, LW), context (1, T, W), time embedding (1, 320) at t = 500."""
    from oracle import rng
    W = MODEL_KINDS[kind]
    lat = rng.normal(7, 800, 4 * LH * LW).reshape(1, 4, LH, LW)
    ctx = rng.normal(7, 801, MODEL_T * W).reshape(1, MODEL_T, W)
    return lat, ctx, ops.time_embedding(500.0).reshape(1, 320)
