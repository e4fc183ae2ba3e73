"""Shared by test_lora_cpu.py and test_gpu_lora.py: operands, the float64 reference of the merge and its bounds, the op wrapper, and
synthetic adapter files in both key dialects.  The reference is `tsd.lora.merge_reference` (float64); nothing here runs on a GPU."""
import ctypes as C

import numpy as np

NEW_ENTRIES = {"tsd_model_lora_add": 8, "tsd_model_lora_clear": 1, "tsd_model_lora_count": 1, "tsd_model_get_param": 4,
               "tsd_debug_model_packed_param": 4, "tsd_lora_merge_f32": 13}
U16 = 2.0 ** -24  # half an ulp of fp32 relative to 1: the unit roundoff of the device's fp32 arithmetic


def exact_operands(O, cols, rows, r, seed):
    """Operands for which every fp32 operation of the merge is exact: W = k / 1024 with |k| < 1024 (an fp16), up / down multiples
    of 1/64 in [-1, 1].  With s in {0.75, -1, 2} and r <= 64 every partial sum is a multiple of 2^-14 below 128: 21 bits."""
    g = np.random.default_rng(seed)
    W = (g.integers(-1023, 1024, size=(O, cols)) / 1024.0).astype(np.float32)
    up = (g.integers(-64, 65, size=(rows, r)) / 64.0).astype(np.float32)
    down = (g.integers(-64, 65, size=(r, cols)) / 64.0).astype(np.float32)
    return W, up, down


def general_operands(O, cols, rows, r, seed):
    """W ~ 0.05 N(0,1) rounded to fp16; up, down ~ 0.1 N(0,1) in fp32."""
    g = np.random.default_rng(seed)
    W = (0.05 * g.standard_normal((O, cols))).astype(np.float16).astype(np.float32)
    up = (0.1 * g.standard_normal((rows, r))).astype(np.float32)
    down = (0.1 * g.standard_normal((r, cols))).astype(np.float32)
    return W, up, down


def gamma(W16, up, down, s):
    """(r + 3) 2^-24 (|W| + |s| sum_j |up||down|): the standard bound for an r-term fp32 dot product in ANY order (r roundings), the
    rounding of s to fp32, its product with the sum and the addition to W (3 more)."""
    r = np.shape(up)[1]
    mag = np.abs(np.asarray(up, np.float64)) @ np.abs(np.asarray(down, np.float64).reshape(np.shape(down)[0], -1))
    W = np.asarray(W16, np.float64)
    return (r + 3) * U16 * (np.abs(W) + abs(float(s)) * mag.reshape(W.shape))


def ulp16(x):
    """Spacing of fp16 at |x| (2^-24 in the subnormal range)."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def check_interval(d, E, g, what):
    """rn16(E - g) <= d <= rn16(E + g) element-wise; prints and returns the worst |d - E| / (ulp16 / 2 + g)."""
    d = np.asarray(d, np.float64)
    lo, hi = np.float16(E - g).astype(np.float64), np.float16(E + g).astype(np.float64)
    worst = float((np.abs(d - E) / (ulp16(E) / 2 + g)).max())
    out = int(((d < lo) | (d > hi)).sum())
    print(f"[lora] {what}: worst |d - E| / (ulp16/2 + gamma) = {worst:.4f}, {out} of {d.size} outside the interval")
    assert out == 0, f"{what}: {out} of {d.size} merged weights leave [rn16(E - gamma), rn16(E + gamma)]"
    return worst


def merge_op(tsd_mod, ctx, W, up, down, s, k=0, interleave=0, row0=0):
    """`tsd_lora_merge_f32` -> (status, out).  W (O, I) for k = 0, (O, I, k, k) otherwise; down (r, I) / (r, I * k * k)."""
    from tsd._lib import ptr
    W, up, down = (np.ascontiguousarray(a, np.float32) for a in (W, up, down))
    out = np.full(W.shape, np.nan, np.float32)
    rc = tsd_mod._lib.lib().tsd_lora_merge_f32(ctx.h if ctx is not None else None, ptr(W), W.shape[0], W.shape[1], k, interleave, row0,
                                               up.shape[0], ptr(up), ptr(down), up.shape[1], float(s), ptr(out))
    return rc, out


# ---- synthetic adapter files ------------------------------------------------------------------------------------------------------
ATTN_SUFFIXES = ["proj_in", "proj_out"] + ["transformer_blocks.0." + s for s in (
    "attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
    "ff.net.0.proj", "ff.net.2")]


def unet_pairs(tsd_mod, modules, rank, seed, amp=0.05):
    """{module: (down, up)} with the shapes a trainer writes for the UNet modules named: conv-shaped (r, I, k, k) / (O, r, 1, 1) for
    convolutions, (r, I) / (O, r) for linear layers."""
    targets = tsd_mod.lora_targets("diffusion_sd15_torch")
    shapes = {n: s for n, s, _, _ in tsd_mod.param_specs("diffusion_sd15_torch")}
    g = np.random.default_rng(seed)
    out = {}
    for mod in modules:
        pname, _, rows = targets[mod]
        shape = shapes[pname]
        dshape = (rank,) + tuple(shape[1:])
        ushape = (rows, rank) + ((1, 1) if len(shape) == 4 else ())
        out[mod] = ((amp * g.standard_normal(dshape)).astype(np.float32), (amp * g.standard_normal(ushape)).astype(np.float32))
    return out


def as_state(pairs, dialect, alpha, prefix="unet"):
    """{key: array} of `pairs` ({module: (down, up)}) in the kohya or the PEFT spelling; prefix "unet" or "text_encoder"."""
    st = {}
    for mod, (down, up) in pairs.items():
        if dialect == "kohya":
            stem = ("lora_unet_" if prefix == "unet" else "lora_te_") + mod.replace(".", "_")
            st[stem + ".lora_down.weight"], st[stem + ".lora_up.weight"] = down, up
        else:
            stem = f"{prefix}.{mod}"
            st[stem + ".lora_A.weight"], st[stem + ".lora_B.weight"] = down, up
        if alpha is not None:
            st[stem + ".alpha"] = np.float32(alpha)
    return st


def attention_modules(tsd_mod):
    """The 16 attention blocks of the SD-1.x UNet (diffusers paths)."""
    from tsd.checkpoint import SD15_MODULES
    return [m for m in SD15_MODULES if ".attentions." in m]
