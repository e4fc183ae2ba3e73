"""Host-side mirror of the reference's `helpers/utils.mojo` layer structs (L1 ops).

Same struct names, constructor arguments and `forward()` meaning as the reference; bodies are one
call into libtsd.so (HIP kernels on gfx950).  Tensors are numpy float32 arrays in the reference's
layout: (C,H,W) images, (1,T,D) or (T,D) token matrices.  Error behaviour mirrors the reference:
shape errors print a message and return a null matrix (`Matrix(0,0,0)`).
"""
import ctypes as C
import math

import numpy as np

from . import _lib, rng
from ._lib import NULL_MATRIX, check, f32, lib, ptr


def _ctx(ctx):
    return (ctx or _lib.default_context()).h


def _tokens(x):
    """(1,T,D) or (T,D) -> (T,D), remembering whether to restore the leading 1."""
    x = f32(x)
    if x.ndim == 3:
        if x.shape[0] != 1:
            raise ValueError("token tensors are (1,T,D) in the reference")
        return x[0], True
    return x, False


class Conv2D:
    """`Conv2D` helpers/utils.mojo:1693-1811: OIHW kernel U(+-1/sqrt(cin*k*k)) (:1722-1724), zero bias (:1717)."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=(0, 0), stride=(1, 1), seed=0, ctx=None):
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.padding, self.stride, self.ctx = tuple(padding), tuple(stride), ctx
        k = in_channels * kernel_size * kernel_size
        self.kernel = rng.uniform(seed, rng.fresh_id(), out_channels * k, 1.0 / math.sqrt(k)).reshape(
            out_channels, in_channels, kernel_size, kernel_size)
        self.bias = np.zeros(out_channels, dtype=np.float32)

    def forward(self, matrix):
        x = f32(matrix)
        C, H, W = x.shape
        ph, pw = self.padding
        sy, sx = self.stride
        k = self.kernel_size
        Ho, Wo = (H + 2 * ph - k) // sy + 1, (W + 2 * pw - k) // sx + 1
        y = np.empty((self.out_channels, max(Ho, 0), max(Wo, 0)), dtype=np.float32)
        code = lib().tsd_conv2d_f32(_ctx(self.ctx), ptr(x), C, H, W, ptr(f32(self.kernel)), ptr(f32(self.bias)),
                                    self.in_channels, self.out_channels, k, ph, pw, sy, sx, ptr(y))
        return NULL_MATRIX() if check(code, True) else y


def pad(matrix, pad_h=(0, 0), pad_w=(0, 0), ctx=None):
    """`Matrix.pad` helpers/utils.mojo:1383-1413."""
    x = f32(matrix)
    C, H, W = x.shape
    y = np.empty((C, H + sum(pad_h), W + sum(pad_w)), dtype=np.float32)
    code = lib().tsd_pad_f32(_ctx(ctx), ptr(x), C, H, W, pad_h[0], pad_h[1], pad_w[0], pad_w[1], ptr(y))
    return NULL_MATRIX() if check(code, True) else y


class GroupNorm:
    """`GroupNorm` helpers/utils.mojo:1813-1885: scalar gamma=1, beta unused, eps added to sigma."""

    def __init__(self, num_groups, num_channels, epsilon=1e-5, ctx=None):
        self.num_groups, self.num_channels, self.epsilon = num_groups, num_channels, epsilon
        self.gamma, self.beta, self.ctx = 1.0, 0.0, ctx

    def forward(self, x):
        x = f32(x)
        C, H, W = x.shape
        y = np.empty((self.num_channels, H, W), dtype=np.float32)
        code = lib().tsd_groupnorm_f32(_ctx(self.ctx), ptr(x), C, H, W, self.num_groups, self.num_channels,
                                       self.epsilon, self.gamma, ptr(y))
        return NULL_MATRIX() if check(code, True) else y


class LayerNorm:
    """`LayerNorm` helpers/utils.mojo:2052-2061 with the build semantics (per-token, SURVEY.md App.A D8)."""

    def __init__(self, n_embed, ctx=None):
        self.n_embed, self.ctx = n_embed, ctx

    def forward(self, x):
        t, lead = _tokens(x)
        y = np.empty_like(t)
        code = lib().tsd_layernorm_f32(_ctx(self.ctx), ptr(t), t.shape[0], t.shape[1], 1e-5, ptr(y))
        if check(code, True):
            return NULL_MATRIX()
        return y[None] if lead else y


def _unary(fn_name, x, ctx):
    x = f32(x)
    y = np.empty_like(x)
    check(getattr(lib(), fn_name)(_ctx(ctx), ptr(x), x.size, ptr(y)))
    return y


class SiLU:
    """`SiLU` helpers/utils.mojo:1888-1902 (pure - App.A D16)."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def forward(self, x):
        return _unary("tsd_silu_f32", x, self.ctx)


class Gelu:
    """`Gelu` helpers/utils.mojo:1904-1919 (tanh approximation)."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def forward(self, x):
        return _unary("tsd_gelu_tanh_f32", x, self.ctx)


class Linear:
    """`Linear` helpers/utils.mojo:1921-1976: weight (out,in), bias (out) allocated always, used iff use_bias.
    Synthetic init U(+-1/sqrt(in)) (App.A D18)."""

    def __init__(self, in_features, out_features, use_bias=True, seed=0, ctx=None):
        self.in_features, self.out_features, self.use_bias, self.ctx = in_features, out_features, use_bias, ctx
        b = 1.0 / math.sqrt(in_features)
        self.weight = rng.uniform(seed, rng.fresh_id(), out_features * in_features, b).reshape(out_features, in_features)
        self.bias = rng.uniform(seed, rng.fresh_id(), out_features, b)

    def forward(self, x):
        t, lead = _tokens(x)
        if t.shape[1] != self.in_features:  # helpers/utils.mojo:1955-1957
            print("Invalid input dimensions for Linear layer. Returning null matrix")
            return NULL_MATRIX()
        y = np.empty((t.shape[0], self.out_features), dtype=np.float32)
        code = lib().tsd_linear_f32(_ctx(self.ctx), ptr(t), t.shape[0], self.in_features, ptr(f32(self.weight)),
                                    ptr(f32(self.bias)) if self.use_bias else None, self.out_features, ptr(y))
        if check(code, True):
            return NULL_MATRIX()
        return y[None] if lead else y


def matmul(a, b, ctx=None):
    """`Matrix.matmul` helpers/utils.mojo:1549-1569: (Ba,M,K) x (Bb,K,N), Bb == 1 broadcasts."""
    a, b = f32(a), f32(b)
    if a.shape[2] != b.shape[1]:  # :1550-1552
        print("Incompatible dimensions for matrix multiplication. Returning null matrix")
        return NULL_MATRIX()
    y = np.empty((a.shape[0], a.shape[1], b.shape[2]), dtype=np.float32)
    code = lib().tsd_matmul_f32(_ctx(ctx), ptr(a), ptr(b), a.shape[0], b.shape[0], a.shape[1], a.shape[2], b.shape[2], ptr(y))
    return NULL_MATRIX() if check(code, True) else y


class Upsample:
    """`Upsample` helpers/utils.mojo:1979-2010, build semantics (App.A D1): nearest x2 whatever `scale_factor`."""

    def __init__(self, scale_factor=1, ctx=None):
        self.scale_factor, self.ctx = scale_factor, ctx

    def forward(self, x):
        if self.scale_factor < 1:  # :1991-1993
            print("Invalid scale factor for upsampling. Returning null matrix")
            return NULL_MATRIX()
        x = f32(x)
        C, H, W = x.shape
        y = np.empty((C, 2 * H, 2 * W), dtype=np.float32)
        check(lib().tsd_upsample_nearest2x_f32(_ctx(self.ctx), ptr(x), C, H, W, ptr(y)))
        return y


def Softmax(matrix, dim=2, ctx=None):
    """`Softmax` helpers/utils.mojo:411-448 as attention uses it; build semantics (App.A D6): last axis."""
    if dim != 2:
        print("Invalid dimension for softmax. Returning null matrix")  # only the attention axis is on the path
        return NULL_MATRIX()
    x = f32(matrix)
    y = np.empty_like(x)
    check(lib().tsd_softmax_lastdim_f32(_ctx(ctx), ptr(x), int(np.prod(x.shape[:-1])), x.shape[-1], ptr(y)))
    return y


def latent_mask(mask, mode="any", ctx=None):
    """Pixel mask (B,8LH,8LW) or (B,1,8LH,8LW) in [0,1] -> latent mask (B,LH,LW) by 8x8 blocks (`tsd_latent_mask_hw_f32`): "area" is the
    block's mean, "any" is 1 where any pixel of the block is >= 0.5 (a cell that touches a masked pixel is regenerated)."""
    m = f32(mask)
    if m.ndim == 4 and m.shape[1] == 1:
        m = np.ascontiguousarray(m[:, 0])
    if m.ndim != 3 or m.shape[1] % 8 or m.shape[2] % 8 or m.shape[1] == 0 or m.shape[2] == 0:
        raise ValueError(f"mask must have shape (B, 8LH, 8LW) or (B, 1, 8LH, 8LW), got {np.shape(mask)}")
    B, LH, LW = m.shape[0], m.shape[1] // 8, m.shape[2] // 8
    y = np.empty((B, LH, LW), dtype=np.float32)
    check(lib().tsd_latent_mask_hw_f32(_ctx(ctx), ptr(m), B, LH, LW, _lib.mask_mode(mode), ptr(y)))
    return y


def normal_fill(seed, stream, n, offset=0, ctx=None):
    """N(0,1) float32 values offset .. offset + n - 1 of the device's counter stream (seed, stream) (`tsd_normal_fill_f32`): what a seeded
    session draws on the device (streams 2 latents, 4 add_noise / inpainting, 16 + i step i).  `rng.normal_counter` is its float64 twin."""
    y = np.empty(int(n), dtype=np.float32)
    mask = (1 << 64) - 1
    check(lib().tsd_normal_fill_f32(_ctx(ctx), int(seed) & mask, int(stream) & mask, int(offset) & mask, int(n), ptr(y)))
    return y


def inpaint_blend(x, mask, known, noise, a_prev, s_prev, ctx=None):
    """x' = m x + (1 - m)(a_prev known + s_prev noise) (`tsd_inpaint_blend_f32`): x / known / noise (B,4,...) and mask (B,...) with one
    value for the 4 channels; noise may be None.  The launch a session with `set_inpaint` adds to a step."""
    x, m, kn = f32(x), f32(mask), f32(known)
    nz = f32(noise) if noise is not None else None
    B = x.shape[0]
    hw = m.size // B if B else 0
    if x.ndim < 2 or x.shape[1] != 4 or m.shape[0] != B or x.size != B * 4 * hw or kn.shape != x.shape or (nz is not None and nz.shape != x.shape):
        raise ValueError(f"inpaint_blend: x {x.shape}, mask {m.shape}, known {kn.shape}" + (f", noise {nz.shape}" if nz is not None else ""))
    y = np.empty_like(x)
    check(lib().tsd_inpaint_blend_f32(_ctx(ctx), ptr(x), ptr(m), ptr(kn), ptr(nz), B, hw, float(a_prev), float(s_prev), ptr(y)))
    return y


def cfg_rescale(eps, eps_uncond, cfg_scale=7.5, phi=0.7, ctx=None):
    """Guidance rescale (`tsd_cfg_rescale_f32`; Lin et al. 2023, eq. 15-16): eps / eps_uncond (B, ...), cfg_scale and phi scalars or one
    value per sample -> (eps', eps_uncond', g) with g (B,) = phi std(eps) / std((eps - eps_uncond) cfg_scale + eps_uncond) + 1 - phi per
    sample and eps' = g eps, eps_uncond' = g eps_uncond.  The launches a session with `set_guidance_rescale` adds to a step."""
    c, u = f32(eps), f32(eps_uncond)
    if c.ndim < 2 or u.shape != c.shape:
        raise ValueError(f"cfg_rescale: eps {c.shape} and eps_uncond {u.shape} must be the same (B, ...) shape")
    B = c.shape[0]
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(cfg_scale, dtype=np.float32), (B,)))
    p = np.ascontiguousarray(np.broadcast_to(np.asarray(phi, dtype=np.float32), (B,)))
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError(f"cfg_rescale: every phi must be between 0 and 1, got {p.tolist()}")
    if not np.isfinite(s).all():
        raise ValueError(f"cfg_rescale: every cfg_scale must be finite, got {s.tolist()}")
    co, uo, g = np.empty_like(c), np.empty_like(u), np.empty(B, dtype=np.float32)
    check(lib().tsd_cfg_rescale_f32(_ctx(ctx), ptr(c), ptr(u), B, c.size // B if B else 0, ptr(s), ptr(p), ptr(co), ptr(uo), ptr(g)))
    return co, uo, g


def ip_attn_add(q, k_ip, vt_ip, o, scale, n_heads, n_tokens, softmax_scale=None, ctx=None):
    """The IP-Adapter's attention launch alone (`tsd_ip_attn_add_f16`): q, o float16 (B, S, C); k_ip float16 (B, 16, C), token-major, rows
    >= n_tokens are not read; vt_ip float16 (B, C, 16), channel-major; scale (B,) ->
    float16(float32(o) + scale_b * softmax(softmax_scale q k_ip^T) v_ip) per head of C / n_heads channels (40, 80 or 160), rounded once.
    softmax_scale defaults to 1 / sqrt(C / n_heads).  A sample whose scale is 0 comes back unchanged."""
    qa, oa = (np.ascontiguousarray(a, dtype=np.float16) for a in (q, o))
    ka, va = (np.ascontiguousarray(a, dtype=np.float16) for a in (k_ip, vt_ip))
    if qa.ndim != 3 or oa.shape != qa.shape:
        raise ValueError(f"ip_attn_add: q {qa.shape} and o {oa.shape} must both be (B, S, C)")
    B, S, Cc = qa.shape
    if ka.shape != (B, 16, Cc) or va.shape != (B, Cc, 16):
        raise ValueError(f"ip_attn_add: k_ip must be ({B}, 16, {Cc}) and vt_ip ({B}, {Cc}, 16), got {ka.shape} and {va.shape}")
    if Cc % int(n_heads):
        raise ValueError(f"ip_attn_add: {n_heads} heads do not divide {Cc} channels")
    d = Cc // int(n_heads)
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float32), (B,)))
    out = np.empty_like(oa)
    sm = 1.0 / math.sqrt(d) if softmax_scale is None else float(softmax_scale)
    check(lib().tsd_ip_attn_add_f16(_ctx(ctx), qa.ctypes.data, ka.ctypes.data, va.ctypes.data, oa.ctypes.data, ptr(s), B, int(n_heads), d, S,
                                    int(n_tokens), sm, out.ctypes.data))
    return out


def control_inject(x, r, scale, groups, nslab, ctx=None):
    """The ControlNet injection launch alone (`tsd_control_inject_f16`) over a table of tensors: x[i], r[i] float16 (B, HW_i, C_i), scale
    (B,), groups[i] / nslab[i] the GroupNorm statistics geometry of tensor i (groups 0: none) -> (y, partial) with
    y[i] = float16(float32(x[i]) + scale_b * float32(r[i])) rounded once and partial[i] float32 (B, nslab_i, groups_i, 2), the (sum, sum of
    squares) of y[i] per slab of ceil(HW_i / nslab_i) rows and channel group (None for an entry without statistics)."""
    xs = [np.ascontiguousarray(a, dtype=np.float16) for a in x]
    rs = [np.ascontiguousarray(a, dtype=np.float16) for a in r]
    n = len(xs)
    if n == 0 or len(rs) != n or len(groups) != n or len(nslab) != n:
        raise ValueError("control_inject: x, r, groups and nslab must be lists of one length")
    B = xs[0].shape[0]
    for a, b in zip(xs, rs):
        if a.ndim != 3 or a.shape != b.shape or a.shape[0] != B:
            raise ValueError(f"control_inject: x {a.shape} and r {b.shape} must both be (B, HW, C) with one B")
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float32), (B,)))
    ys = [np.empty_like(a) for a in xs]
    ps = [np.empty((B, int(ns), int(g), 2), dtype=np.float32) if g else None for g, ns in zip(groups, nslab)]
    I, V = C.c_int * n, C.c_void_p * n
    vp_of = lambda arrs: V(*[a.ctypes.data for a in arrs])  # noqa: E731
    parts = (_lib.fp * n)(*[ptr(p) if p is not None else None for p in ps])
    check(lib().tsd_control_inject_f16(_ctx(ctx), n, vp_of(xs), vp_of(rs), B, I(*[a.shape[1] for a in xs]), I(*[a.shape[2] for a in xs]),
                                       I(*[int(g) for g in groups]), I(*[int(v) for v in nslab]), ptr(s), vp_of(ys), parts))
    return ys, ps


def ddpm_step(x, eps, eps_uncond, cfg_scale, noise, i, num_inference_steps, num_training_steps=1000, start_step=0, spacing="leading",
              ctx=None):
    """The update of step i of a DDPM session with this schedule (`tsd_ddpm_step_f32`) on host tensors; eps_uncond and noise may be None."""
    x, e = f32(x), f32(eps)
    u = f32(eps_uncond) if eps_uncond is not None else None
    z = f32(noise) if noise is not None else None
    if e.shape != x.shape or (u is not None and u.shape != x.shape) or (z is not None and z.shape != x.shape):
        raise ValueError(f"ddpm_step: x {x.shape}, eps {e.shape} and the optional tensors must have one shape")
    y = np.empty_like(x)
    check(lib().tsd_ddpm_step_f32(_ctx(ctx), ptr(x), ptr(e), ptr(u), float(cfg_scale), ptr(z), x.size, _lib.timestep_spacing(spacing),
                                  int(num_training_steps), int(num_inference_steps), int(start_step), int(i), ptr(y)))
    return y


def sampler_step_v(x, v, v_uncond, cfg_scale, hist, noise, c, want_hist=True, ctx=None):
    """One update of a v-prediction session (`tsd_sampler_step_v_f32`) on host tensors with the scalars c = (alpha_t, sigma_t, c_x, c_v,
    c_h, c_n), e.g. out[2:] of `tsd_sampler_coeffs_ex`: -> (x', h') with h' = alpha_t x - sigma_t v the data prediction (None without
    want_hist).  v_uncond, hist and noise may be None: the term is skipped."""
    x, vv = f32(x), f32(v)
    u, h, z = (f32(a) if a is not None else None for a in (v_uncond, hist, noise))
    if vv.shape != x.shape or any(a is not None and a.shape != x.shape for a in (u, h, z)):
        raise ValueError(f"sampler_step_v: x {x.shape}, v {vv.shape} and the optional tensors must have one shape")
    c6 = np.ascontiguousarray(np.asarray(c, dtype=np.float32).reshape(-1))
    if c6.size != 6:
        raise ValueError(f"sampler_step_v: c must hold the 6 scalars (alpha_t, sigma_t, c_x, c_v, c_h, c_n), got {c6.size}")
    y = np.empty_like(x)
    ho = np.empty_like(x) if want_hist else None
    check(lib().tsd_sampler_step_v_f32(_ctx(ctx), ptr(x), ptr(vv), ptr(u), float(cfg_scale), ptr(h), ptr(z), x.size, ptr(c6), ptr(y), ptr(ho)))
    return y, ho


def alphas_cumprod(num_training_steps=1000, zero_terminal_snr=False):
    """The alphas_cumprod table a session runs on (`tsd_sampler_alphas_cumprod`, host only): the reference's fp32 table, or its
    zero-terminal-SNR rescale (Lin et al. 2023, algorithm 1), whose last entry is exactly 0."""
    n = int(num_training_steps)
    out = np.empty(max(n, 0), dtype=np.float32)
    rc = lib().tsd_sampler_alphas_cumprod(n, 1 if zero_terminal_snr else 0, ptr(out), n)
    if rc < 0:
        check(rc)
    return out


def get_time_embedding(timestep, ctx=None):
    """`get_time_embedding` helpers/utils.mojo:353-370 -> (1,1,320)."""
    y = np.empty(320, dtype=np.float32)
    check(lib().tsd_time_embedding_f32(_ctx(ctx), float(timestep), ptr(y)))
    return y.reshape(1, 1, 320)


def concat(a, b, dim=0):
    """`Matrix.concat` helpers/utils.mojo:605-647 (host glue, like the reference's Matrix method)."""
    return np.concatenate([f32(a), f32(b)], axis=dim)


def rescale(x, old_scale, new_scale, clamp=False):
    """`Matrix.rescale` helpers/utils.mojo:577-597 (host glue; pipeline.mojo:70,127)."""
    o0, o1 = old_scale
    n0, n1 = new_scale
    y = (f32(x) - o0) * (n1 - n0) / (o1 - o0) + n0
    return np.clip(y, n0, n1).astype(np.float32) if clamp else y.astype(np.float32)
