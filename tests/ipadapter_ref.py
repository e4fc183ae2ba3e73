"""Reference for the IP-Adapter: the kernel k_ip_attn_add (csrc/kernels_ipattn.hip) element-wise, and the adapted UNet forward.

TEST INFRASTRUCTURE.  Three statements of the kernel:

  reference()  fp64:   y = o + s_b * sum_j softmax_j(scale * q . k_j) v_j   over the N live keys of every (sample, head, query)
  emulate()    numpy with the kernel's rounding points: fp32 scores, fp32 scale and max subtraction, fp32 exp, p rounded to fp16, the
               denominator the fp32 sum of the rounded p, fp32 P.V, one division, one fma with s_b (rounded to fp32, then to fp16)
  bound()      an element-wise bound on |kernel - reference|, a function of the inputs alone, DERIVED from those rounding points.

The bound.  u16 = 2^-11, u32 = 2^-24, gamma_n = n u32 / (1 - n u32).  For one query and head, z_j = scale (q . k_j) exactly, m = max z,
W_j = exp(z_j - m), D = sum W_j >= 1, R = sum W_j v_j / D.
  1. scores: fp16 x fp16 products are exact in fp32; accumulated in fp32 over dpad terms (the matrix unit's order is not specified, so the
     worst case over all orders): |err| <= gamma_dpad A_j with A_j = sum_c |q_c k_jc|; the multiplication by scale adds u32 |z_j|:
         a_j = scale gamma_dpad A_j + u32 |z_j|,   amax = max_j a_j   (the computed maximum is off by at most amax)
  2. the subtraction of the maximum: u32 (|z_j - m| + amax).  A shift common to all keys cancels in the ratio, so the exponent of key j
     is off, relative to the others, by  dl_j = a_j + amax + u32 (|z_j - m| + amax).
  3. the device exponential: EXP_ULPS ulps, eps_exp = EXP_ULPS 2^-23; the rounding of p_j to fp16: u16 relative, or 2^-25 absolute
     where p_j is subnormal.  Hence p_j / c = W_j + e_j (c the common factor) with
         |e_j| <= E_j = W_j (exp(dl_j) (1 + eps_exp) (1 + u16) - 1) + 2^-25 exp(amax)
  4. the ratio with exact arithmetic on the rounded p:  |R' - R| = |sum e_j (v_j - R)| / sum (W_j + e_j) <= sum E_j |v_j - R| / (D - sum E_j)
  5. fp32 arithmetic: the numerator accumulates 16 exact products (gamma_16), the denominator is a sum of depth 4 (gamma_4: an in-lane
     pair of adds and two cross-lane adds), one division (u32):   |t - R'| <= (gamma_16 + gamma_4 + 2 u32) Vmax (1 + 2^-10),  Vmax = max_j |v_j|
  6. the fma with s_b rounds to fp32 and the result to fp16:  (u16 + 2 u32) |y| + 2^-25 (subnormal results)
  bound = E_in + (u16 + 2 u32) (|y_ref| + E_in) + 2^-25,   E_in = |s_b| (step 4 + step 5)
It is not tuned to a measurement: a case that exceeds it means the kernel or this derivation is wrong.
"""
import math

import numpy as np

import replay

U16, U32 = 2.0 ** -11, 2.0 ** -24
EXP_ULPS = 4.0
TOKENS = 16  # token rows of K_ip / columns of V_ip^T that exist, whatever N is

_HDR = replay.header()
PD, PO, PI = replay.enums(_HDR, {"TSD_PD_": "tsd_ipattn_desc_field", "TSD_PO_": "tsd_ipattn_operand", "TSD_PI_": "tsd_ipattn_info"})
VERSION = replay.version(_HDR, "TSD_PD_VERSION_1")
INPUTS = ("Q", "K", "VT", "S", "OIN")


def F(d, k):
    return int(d[PD[k]])


def desc(B, H, hd, S, N, gap=8, scale=None, sgap=16):
    """Descriptor with pitches `gap` elements wider than C (q and o; 0: dense) and per-sample strides `sgap` elements past the rows."""
    C = H * hd
    d = np.zeros(PD["COUNT"], np.int64)
    d[PD["VERSION"]] = VERSION
    d[PD["B"]], d[PD["H"]], d[PD["D"]], d[PD["S"]], d[PD["N"]] = B, H, hd, S, N
    d[PD["LDQ"]], d[PD["LDK"]], d[PD["LDVT"]], d[PD["LDO"]] = C + gap, C, TOKENS, C + 2 * gap
    d[PD["SQB"]] = max(S, 1) * d[PD["LDQ"]] + sgap
    d[PD["SKB"]] = TOKENS * d[PD["LDK"]]
    d[PD["SVTB"]] = C * d[PD["LDVT"]]
    d[PD["SOB"]] = max(S, 1) * d[PD["LDO"]] + sgap
    d[PD["SCALE"]] = replay.f32_bits(1.0 / math.sqrt(hd) if scale is None else scale)
    return d


def scale_of(d):
    return replay.bits_f32(F(d, "SCALE"))


def dtype_of(s, d):
    return np.float32 if s == "S" else np.float16


def extents(d):
    B, C, S = F(d, "B"), F(d, "H") * F(d, "D"), max(F(d, "S"), 1)
    o = (B - 1) * F(d, "SOB") + (S - 1) * F(d, "LDO") + C
    return {"Q": (B - 1) * F(d, "SQB") + (S - 1) * F(d, "LDQ") + C, "K": (B - 1) * F(d, "SKB") + (TOKENS - 1) * F(d, "LDK") + C,
            "VT": (B - 1) * F(d, "SVTB") + (C - 1) * F(d, "LDVT") + TOKENS, "S": B, "OIN": o, "O": o}


def _index(d, sb, ld, rows):
    B, C = F(d, "B"), F(d, "H") * F(d, "D")
    return (np.arange(B)[:, None, None] * F(d, sb) + np.arange(rows)[None, :, None] * F(d, ld) + np.arange(C)[None, None, :])


def o_index(d):
    return _index(d, "SOB", "LDO", F(d, "S"))


def pack(d, q, k, vt, o, s, fill=replay.NAN16):
    """q, o (B, S, C); k (B, 16, C) token-major; vt (B, C, 16) channel-major; s (B,) -> the flat operands in their device layout, the
    pitch gaps of q and o holding the fill."""
    e = extents(d)
    ops = {n: np.full(e[n], fill, np.float16) for n in ("Q", "OIN")}
    ops["Q"][_index(d, "SQB", "LDQ", F(d, "S"))] = q.astype(np.float16)
    ops["OIN"][o_index(d)] = o.astype(np.float16)
    ops["K"] = np.ascontiguousarray(k, np.float16).reshape(-1)
    ops["VT"] = np.ascontiguousarray(vt, np.float16).reshape(-1)
    ops["S"] = np.ascontiguousarray(s, np.float32)
    assert all(ops[n].size == e[n] for n in INPUTS)
    return ops


def unpack(d, ops):
    B, C, S = F(d, "B"), F(d, "H") * F(d, "D"), F(d, "S")
    q = ops["Q"][_index(d, "SQB", "LDQ", S)]
    o = ops["OIN"][o_index(d)]
    return q, ops["K"].reshape(B, TOKENS, C), ops["VT"].reshape(B, C, TOKENS), o, ops["S"]


def unpack_output(d, y):
    return y[o_index(d)]


def _heads(d, ops, dt):
    """q (B,H,S,hd), k (B,H,N,hd), v (B,H,N,hd), o (B,H,S,hd), s (B,) as dt - the N live keys only."""
    B, H, hd, S, N = (F(d, k) for k in ("B", "H", "D", "S", "N"))
    q, k, vt, o, s = unpack(d, ops)
    qh = q.astype(dt).reshape(B, S, H, hd).transpose(0, 2, 1, 3)
    kh = k[:, :N].astype(dt).reshape(B, N, H, hd).transpose(0, 2, 1, 3)
    vh = vt[:, :, :N].astype(dt).reshape(B, H, hd, N).transpose(0, 1, 3, 2)
    oh = o.astype(dt).reshape(B, S, H, hd).transpose(0, 2, 1, 3)
    return qh, kh, vh, oh, s.astype(dt)


def _merge(d, y):
    B, H, hd, S = (F(d, k) for k in ("B", "H", "D", "S"))
    return y.transpose(0, 2, 1, 3).reshape(B, S, H * hd)


def reference(d, ops):
    """fp64 statement of the formula -> (B, S, C) float64.  A sample whose scale is 0 is its input."""
    q, k, v, o, s = _heads(d, ops, np.float64)
    z = np.float64(scale_of(d)) * (q @ k.transpose(0, 1, 3, 2))
    w = np.exp(z - z.max(-1, keepdims=True))
    r = (w @ v) / w.sum(-1, keepdims=True)
    return _merge(d, o + s[:, None, None, None] * r)


def emulate(d, ops):
    """The kernel's rounding points in numpy -> (B, S, C) float16."""
    q, k, v, o, s = _heads(d, ops, np.float32)
    z = (q @ k.transpose(0, 1, 3, 2)).astype(np.float32) * np.float32(scale_of(d))
    e = np.exp((z - z.max(-1, keepdims=True)).astype(np.float32)).astype(np.float32)
    p = e.astype(np.float16).astype(np.float32)
    den = np.zeros(p.shape[:-1] + (1,), np.float32)
    for j in range(p.shape[-1]):
        den = (den + p[..., j:j + 1]).astype(np.float32)
    t = ((p @ v).astype(np.float32) / den).astype(np.float32)
    y = (o.astype(np.float64) + s.astype(np.float64)[:, None, None, None] * t.astype(np.float64)).astype(np.float32).astype(np.float16)
    y = np.where((s == 0)[:, None, None, None], o.astype(np.float16), y)
    return _merge(d, y)


def _gamma(n):
    return n * U32 / (1.0 - n * U32)


def dpad_of(hd):
    return (hd + 31) // 32 * 32


def bound(d, ops):
    """Element-wise bound on |kernel - reference| (module docstring) -> (B, S, C) float64; 0 for a sample whose scale is 0."""
    q, k, v, o, s = _heads(d, ops, np.float64)
    sc = float(scale_of(d))
    z = sc * (q @ k.transpose(0, 1, 3, 2))                      # (B,H,S,N)
    A = np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2)
    a = sc * _gamma(dpad_of(F(d, "D"))) * A + U32 * np.abs(z)
    amax = a.max(-1, keepdims=True)
    m = z.max(-1, keepdims=True)
    dl = a + amax + U32 * (np.abs(z - m) + amax)
    W = np.exp(z - m)
    D = W.sum(-1, keepdims=True)
    E = W * (np.exp(dl) * (1 + EXP_ULPS * 2.0 ** -23) * (1 + U16) - 1) + 2.0 ** -25 * np.exp(amax)
    R = (W @ v) / D                                             # (B,H,S,hd)
    dev = np.abs(v[:, :, None, :, :] - R[:, :, :, None, :])     # (B,H,S,N,hd): |v_j - R|
    step4 = (E[..., None] * dev).sum(-2) / (D - E.sum(-1, keepdims=True))
    vmax = np.abs(v).max(-2)[:, :, None, :]                     # (B,H,1,hd)
    step5 = (_gamma(16) + _gamma(4) + 2 * U32) * vmax * (1 + 2.0 ** -10)
    sb = np.abs(s)[:, None, None, None]
    e_in = sb * (step4 + step5)
    y = o + s[:, None, None, None] * R
    b = e_in + (U16 + 2 * U32) * (np.abs(y) + e_in) + 2.0 ** -25
    return _merge(d, np.where(sb == 0, 0.0, b))


def well_conditioned(d, ops):
    """The scores leave the fp16 range of p alone (|z - m| small enough that exp is a normal fp16) and nothing is near overflow."""
    q, k, v, o, s = _heads(d, ops, np.float64)
    z = float(scale_of(d)) * (q @ k.transpose(0, 1, 3, 2))
    return bool((z.max(-1) - z.min(-1)).max() < 9.0 and np.abs(o).max() + np.abs(s).max() * np.abs(v).max() < 60000.0)


def check(d, ops, out_flat, ref=None):
    """(list of failures, worst error / bound) of a flat kernel output against the reference."""
    y = unpack_output(d, out_flat).astype(np.float64)
    ref = reference(d, ops) if ref is None else ref
    b = bound(d, ops)
    err = np.abs(y - ref)
    fails = []
    if not np.isfinite(y).all():
        fails.append("non-finite output")
    bad = err > b
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(b, 1e-300), 0)), err.shape)
        fails.append(f"{int(bad.sum())} elements outside the bound; worst at {i}: |err| {err[i]:.3e} > {b[i]:.3e}")
    live = b > 0
    ratio = float((err[live] / b[live]).max()) if live.any() else 0.0
    return fails, ratio


def make_inputs(d, seed=0, scales=None, span=None, pad=0.0):
    """Well-conditioned operands: q, k ~ N(0, 1) scaled so that the scores spread over a few units, v, o ~ N(0, 1).  span: the scores of
    every query are spread over `span` natural-log units instead (keys on a line), so the smallest p underflow.  pad: what rows N .. 15
    of K_ip and columns N .. 15 of V_ip^T hold."""
    B, H, hd, S, N = (F(d, k) for k in ("B", "H", "D", "S", "N"))
    C = H * hd
    r = np.random.default_rng(seed)
    q = r.standard_normal((B, S, C))
    k = np.full((B, TOKENS, C), pad, np.float64)
    k[:, :N] = r.standard_normal((B, N, C))
    if span is not None:  # key j = j * step along the query's mean direction: scores differ by ~ span / (N - 1) per key
        u = np.ones(hd) / math.sqrt(hd)
        q = np.tile(u * 4.0, (B, S, H)) + 0.05 * q
        for j in range(N):
            k[:, j] = np.tile(u, H) * (j * span / max(N - 1, 1)) / (4.0 * scale_of(d)) + 0.05 * k[:, j]
    vt = np.full((B, C, TOKENS), pad, np.float64)
    vt[:, :, :N] = r.standard_normal((B, C, N))
    o = r.standard_normal((B, S, C))
    s = np.asarray(scales if scales is not None else [1.0] * B, np.float32)
    return pack(d, q, k, vt, o, s)


# ---- model level: the image projection and the adapted UNet forward, from the restatement controlnet_ref builds on ---------------------
def published_index(t):
    """`ip_adapter.<i>` of the t-th cross-attention block of the step table (6 down, 1 mid, 9 up)."""
    return 2 * t + 1 if t < 6 else (31 if t == 6 else 2 * t - 1)


def project(P, embeds, n_tokens=4):
    """(B, 1024) -> (B, n_tokens, 768): LayerNorm(Linear(e)) per token, eps 1e-5, in fp64."""
    e = np.asarray(embeds, np.float64)
    y = e @ np.asarray(P["image_proj.proj.weight"], np.float64).T + np.asarray(P["image_proj.proj.bias"], np.float64)
    y = y.reshape(e.shape[0], n_tokens, 768)
    mu, var = y.mean(-1, keepdims=True), y.var(-1, keepdims=True)
    return ((y - mu) / np.sqrt(var + 1e-5) * np.asarray(P["image_proj.norm.weight"], np.float64)
            + np.asarray(P["image_proj.norm.bias"], np.float64)).astype(np.float32)


class adapted:
    """Context manager: while it is open, oracle.ops.cross_attention adds s * Attn(q, tok Wk_ip^T, tok Wv_ip^T) to the text attention
    before the output projection in every block whose k_proj weight belongs to `unet_params` - so oracle.models.diffusion_sd15 and
    controlnet_ref.diffusion_sd15_controlled restate the adapted forward.  One sample: tokens (N, 768), scale a float."""

    def __init__(self, unet_params, ip_params, tokens, scale):
        from oracle.spec import FULL_UNET_STEPS
        self.map, t = {}, 0
        for i, (kind, _, _) in enumerate(FULL_UNET_STEPS, start=1):
            if kind != "attn":
                continue
            n = f"ip_adapter.{published_index(t)}"
            self.map[id(unet_params[f"unet.layer{i}.layer6.k_proj.weight"])] = (ip_params[n + ".to_k_ip.weight"], ip_params[n + ".to_v_ip.weight"])
            t += 1
        assert t == 16
        self.tokens, self.scale = np.asarray(tokens, np.float32), np.float32(scale)

    def __enter__(self):
        from oracle import ops
        self.ops, self.orig = ops, ops.cross_attention
        me = self

        def cross_attention(x, ctx, H, wq, bq, wk, bk, wv, bv, wo, bo, sem=ops.DEFAULT):
            if id(wk) not in me.map:
                return me.orig(x, ctx, H, wq, bq, wk, bk, wv, bv, wo, bo, sem=sem)
            wki, wvi = me.map[id(wk)]
            q = ops.linear(x, wq, bq)
            text = ops.attention_core(q, ops.linear(ctx, wk, bk), ops.linear(ctx, wv, bv), H, False, sem)
            tok = me.tokens.astype(x.dtype)
            img = ops.attention_core(q, ops.linear(tok, wki.astype(x.dtype)), ops.linear(tok, wvi.astype(x.dtype)), H, False, sem)
            return ops.linear(text + me.scale.astype(x.dtype) * img, wo, bo)
        ops.cross_attention = cross_attention
        return self

    def __exit__(self, *exc):
        self.ops.cross_attention = self.orig
        return False
