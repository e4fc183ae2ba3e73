"""fp64 restatement of the CLIP vision encoder (model kind "clip_vision_h") and of its image front end, with the derived error bound of
the front-end kernel.

TEST INFRASTRUCTURE.  Three parts:

1. The image front end (k_clip_image_patches, csrc/kernels_vision.hip) as the float-valued form of Hugging Face's CLIPImageProcessor:
   resize (shortest edge to 224, the other edge to int(224 * long / short), PIL's separable antialiased bicubic, horizontal pass first),
   centre crop to 224 x 224, (v / 255 - mean) / std, the patch layout [256][588] with column c * 196 + kh * 14 + kw.  Everything in
   fp64: `axis_table`, `resize_crop`, `patches`.
2. `bound`: what the kernel may differ from part 1 by, element for element (derived below).
3. `encoder`: the transformer on top, with its dimensions as arguments so that a CPU test can hold it to an independent torch
   restatement at a reduced size and the GPU test can run it at full size.  Linear layers, the attention core and the softmax are
   oracle.ops'; LayerNorm and erf-GELU restate ops.layer_norm_torch / ops.gelu_erf without their final cast to fp32, so that an fp64 run
   stays fp64.

THE BOUND.  An output element is  y = a_c v + b_c,  a_c = 1 / (255 std_c),  b_c = -mean_c / std_c,  with
    v = sum_s w_v[s] * ( sum_t w_h[t] * x[s][t] )          T_v vertical taps, T_h horizontal taps, x the fp32 pixels.
The kernel holds the coefficients rounded to fp32 and sums in fp32 with one fma per tap.  With u = 2^-24:
  * a horizontal sum of T_h terms, each coefficient carrying one rounding (1 + d), |d| <= u, and each of the T_h fmas another, differs from
    the exact one by at most gamma(T_h + 1) sum_t |w_h[t]| |x[s][t]|  (gamma(n) = n u / (1 - n u); any order of summation);
  * the vertical sum does the same to its inputs: T_v + 1 more roundings on every path from a pixel to v.
  Together  |v^ - v| <= gamma(T_h + T_v + 2) A,  A = sum_s |w_v[s]| sum_t |w_h[t]| |x[s][t]|;  for T_h + T_v + 2 <= 80,
  gamma(n) <= 1.01 n u  (n u < 5e-6), which is the form used:   E_v = 1.01 (T_h + T_v + 2) u A.
  * the normalisation is one fma on constants rounded to fp32: y^ = (a_c (1 + d1) v^ + b_c (1 + d2)) (1 + d3).  The error of v^ passes
    through scaled by a_c; the three roundings add at most u |a_c v| + u |b_c| + u |y| <= 2 u (|v| / (255 std_c) + mean_c / std_c)
    (|y| <= |a_c v| + |b_c|; terms in u^2 are below the slack of the 1.01 above);
  * the store rounds once to fp16: half an ulp, at most 2^-11 |y| for a normal result and 2^-25 below 2^-14.
      bound = E_v / (255 std_c) + 2 u (|v| / (255 std_c) + mean_c / std_c) + max(2^-11 |y|, 2^-25)
The last term dominates (4.9e-4 |y| against ~1e-6): a worst ratio near 1 is a half-ulp rounding, a ratio above 1 a wrong value.
"""
import numpy as np

from oracle import ops

SIDE, PATCH, GRID, NPATCH, PATCH_K, PATCH_LD = 224, 14, 16, 256, 588, 592
MEAN = np.array([0.48145466, 0.4578275, 0.40821073], np.float64)
STD = np.array([0.26862954, 0.26130258, 0.27577711], np.float64)
U32 = 2.0 ** -24


# ---- 1. the front end in fp64 -----------------------------------------------------------------------------------------------------------
def keys_cubic(x, a=-0.5):
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def resized_size(H, W):
    """(RH, RW): the shortest edge goes to 224, the other one to int(224 * long / short)."""
    if H <= W:
        return SIDE, int(SIDE * W / H)
    return int(SIDE * H / W), SIDE


def crop_offsets(H, W):
    RH, RW = resized_size(H, W)
    return (RH - SIDE) // 2, (RW - SIDE) // 2


def axis_table(n_in, n_out, off=0, count=None):
    """[(lo, weights fp64)] for outputs off .. off + count - 1 of the resize of n_in samples to n_out (PIL's precompute_coeffs)."""
    count = n_out - off if count is None else count
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    out = []
    for xx in range(off, off + count):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = keys_cubic((np.arange(lo, hi) - center + 0.5) / fs)
        out.append((lo, w / w.sum()))
    return out


def dense(table, n_in):
    """The table as a [len(table)][n_in] matrix, and the tap count of every row."""
    m = np.zeros((len(table), n_in), np.float64)
    for o, (lo, w) in enumerate(table):
        m[o, lo:lo + len(w)] = w
    return m, np.array([len(w) for _, w in table])


def tables(H, W):
    """(Wy [224][H], taps_y [224], Wx [224][W], taps_x [224]): the coefficient rows of the 224 cropped outputs of each axis."""
    RH, RW = resized_size(H, W)
    top, left = crop_offsets(H, W)
    wy, ty = dense(axis_table(H, RH, top, SIDE), H)
    wx, tx = dense(axis_table(W, RW, left, SIDE), W)
    return wy, ty, wx, tx


def resize_crop(img, with_abs=False):
    """img [3][H][W] (0 .. 255) -> fp64 [3][224][224]; with_abs: also A = |Wy| |x| |Wx|^T and the tap counts (T_v [224], T_h [224])."""
    x = np.asarray(img, np.float64)
    wy, ty, wx, tx = tables(x.shape[1], x.shape[2])
    v = np.einsum("yh,chw->cyw", wy, x @ wx.T)       # horizontal pass first, then vertical
    if not with_abs:
        return v
    a = np.einsum("yh,chw->cyw", np.abs(wy), np.abs(x) @ np.abs(wx).T)
    return v, a, ty, tx


def to_patches(t):
    """[3][224][224] -> [256][588]: row py * 16 + px, column c * 196 + kh * 14 + kw."""
    return t.reshape(3, GRID, PATCH, GRID, PATCH).transpose(1, 3, 0, 2, 4).reshape(NPATCH, PATCH_K)


def normalise(v):
    return (v / 255.0 - MEAN[:, None, None]) / STD[:, None, None]


def patches(img):
    """fp64 reference of the front end for one image: [256][588]."""
    return to_patches(normalise(resize_crop(img)))


def bound(img):
    """(reference [256][588], bound [256][588]) for one fp32 image: see THE BOUND in the module docstring."""
    v, a, ty, tx = resize_crop(np.asarray(img, np.float32), with_abs=True)
    n = (ty[:, None] + tx[None, :] + 2).astype(np.float64)[None]
    assert n.max() <= 80
    ev = 1.01 * n * U32 * a
    s = (255.0 * STD)[:, None, None]
    y = normalise(v)
    b = ev / s + 2.0 * U32 * (np.abs(v) / s + (MEAN / STD)[:, None, None]) + np.maximum(2.0 ** -11 * np.abs(y), 2.0 ** -25)
    return to_patches(y), to_patches(b)


# ---- 3. the encoder ---------------------------------------------------------------------------------------------------------------------
def _layer_norm(x, w, b, eps=1e-5):   # ops.layer_norm_torch, the result kept in x's dtype
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=-1, keepdims=True)
    var = x64.var(axis=-1, keepdims=True)
    return ((x64 - mu) / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)).astype(x.dtype)


def _gelu_erf(x):                     # ops.gelu_erf, the result kept in x's dtype
    from scipy.special import erf
    x64 = x.astype(np.float64)
    return (0.5 * x64 * (1.0 + erf(x64 / np.sqrt(2.0)))).astype(x.dtype)


def encoder(P, patch_rows, heads, layers, dtype=np.float64):
    """patch_rows [n_patches][K] (the front end's rows, K = the patch embedding's fan-in) -> (image_embeds [E], hidden [1 + n_patches][D]):
    HF's CLIPVisionModelWithProjection on kind "clip_vision_h"'s parameter names.  hidden is the input of the last layer
    (hidden_states[-2]).  Width, token count, MLP width and projection width come from the parameters' shapes."""
    p = lambda k: np.asarray(P[k], dtype)  # noqa: E731
    x = ops.linear(np.asarray(patch_rows, dtype), p("embeddings.patch_embedding.weight"))
    x = np.concatenate([p("embeddings.class_embedding")[None], x]) + p("embeddings.position_embedding.weight")
    x = _layer_norm(x, P["pre_layrnorm.weight"], P["pre_layrnorm.bias"])
    hidden = None
    for i in range(layers):
        n = f"layers.{i}"
        if i == layers - 1:
            hidden = x
        h = _layer_norm(x, P[n + ".ln1.weight"], P[n + ".ln1.bias"])
        x = x + ops.self_attention(h, heads, p(n + ".in_proj.weight"), p(n + ".in_proj.bias"), p(n + ".out_proj.weight"), p(n + ".out_proj.bias"))
        h = _layer_norm(x, P[n + ".ln2.weight"], P[n + ".ln2.bias"])
        h = _gelu_erf(ops.linear(h, p(n + ".fc1.weight"), p(n + ".fc1.bias")))
        x = x + ops.linear(h, p(n + ".fc2.weight"), p(n + ".fc2.bias"))
    pooled = _layer_norm(x[:1], P["post_layernorm.weight"], P["post_layernorm.bias"])
    return ops.linear(pooled, p("visual_projection.weight"))[0], hidden


def clip_vision_h(P, img, dtype=np.float32):
    """One image [3][H][W] on 0 .. 255 through the full-size encoder: (image_embeds [1024], hidden [257][1280])."""
    return encoder(P, patches(img), 16, 32, dtype)


def reduced_specs(width=64, layers=2, patch_k=27, tokens=10, mlp=128, embed=32):
    """Kind "clip_vision_h"'s inventory at other dimensions: [(name, shape)] in the library's order."""
    out = [("embeddings.class_embedding", (width,)), ("embeddings.patch_embedding.weight", (width, patch_k)),
           ("embeddings.position_embedding.weight", (tokens, width)), ("pre_layrnorm.weight", (width,)), ("pre_layrnorm.bias", (width,))]
    for i in range(layers):
        n = f"layers.{i}"
        out += [(n + ".ln1.weight", (width,)), (n + ".ln1.bias", (width,)), (n + ".in_proj.weight", (3 * width, width)), (n + ".in_proj.bias", (3 * width,)),
                (n + ".out_proj.weight", (width, width)), (n + ".out_proj.bias", (width,)), (n + ".ln2.weight", (width,)), (n + ".ln2.bias", (width,)),
                (n + ".fc1.weight", (mlp, width)), (n + ".fc1.bias", (mlp,)), (n + ".fc2.weight", (width, mlp)), (n + ".fc2.bias", (width,))]
    return out + [("post_layernorm.weight", (width,)), ("post_layernorm.bias", (width,)), ("visual_projection.weight", (embed, width))]


# ---- the replay entry's descriptor (tsd_debug_image_patches_run) --------------------------------------------------------------------------
def enums():
    import replay
    return replay.enums(replay.header(), {"TSD_VD_": "tsd_imgpatch_desc_field", "TSD_VO_": "tsd_imgpatch_operand", "TSD_VI_": "tsd_imgpatch_info"})


def desc(B, H, W, ld=PATCH_LD):
    import replay
    VD, _, _ = enums()
    d = np.zeros(VD["COUNT"], np.int64)
    d[VD["VERSION"]] = replay.version(replay.header(), "TSD_VD_VERSION_1")
    d[VD["B"]], d[VD["H"]], d[VD["W"]], d[VD["LD"]] = B, H, W, ld
    return d


def extents(d):
    VD, _, _ = enums()
    return {"IMG": int(d[VD["B"]] * 3 * d[VD["H"]] * d[VD["W"]]), "OUT": int(d[VD["B"]] * NPATCH * d[VD["LD"]])}


def run(ctx, images, ld=PATCH_LD, unsizable_ok=False):
    """images fp32 [B][3][H][W] through the guarded replay entry: (status, fp16 [B][256][ld] or None, info dict)."""
    import replay
    VD, VO, VI = enums()
    img = np.ascontiguousarray(images, np.float32)
    B, _, H, W = img.shape
    d = desc(B, H, W, ld)
    rc, outs, info = replay.run("tsd_debug_image_patches_run", ctx, d, {"IMG": img.reshape(-1)}, VO, ("IMG",), ("OUT",),
                                lambda s, _d: np.float32 if s == "IMG" else np.float16, extents, unsizable_ok=unsizable_ok)
    if outs is None:
        return rc, None, None
    return rc, outs["OUT"].reshape(B, NPATCH, ld), {k: int(info[v]) for k, v in VI.items() if k != "COUNT"}
