"""fp64 reference and element-wise check for the time path, the activations, the boundary conversions and the packers of
csrc/kernels_elementwise.hip (test infrastructure).

A launch is a descriptor: the int64 TSD_ED_* fields of include/tsd.h (parsed from the header), one per argument of the launch_*
function its mode names.  Operands are flat numpy arrays in the device layout - pitch gaps hold the NaN fill, so an over-read shows as a
non-finite output - exactly what tsd_debug_elem_run uploads.  `reference(d, ops)` is float64 on the exact input bits and literal to the
formula written beside each kernel; `check` holds an output to it.

Pure movement plus one rounding (the layout conversions, the packers, the row converters, CLIP_EMBED): no tolerance.  The expected
bits are numpy's own round-to-nearest-even - astype(float16) of the float32 product with `scale`, of the float32 sum for CLIP_EMBED -
and `check` compares bit patterns.  The inputs are value-coded (`coded16`): element i holds the i-th fp16 bit pattern of a fixed walk
through the normal range, so every source element is distinct, survives the rounding and names its own index; a handful of fp32
sources are then replaced by rounding ties, values beyond 65504 and values that are subnormal in fp16 (`SPECIALS`).

Bounds of the arithmetic kernels, u = 2^-24, h = 2^-11 (one fp16 rounding: h |ref| + 2^-25, the 2^-25 for fp16's subnormal range):

  * SMALL_LINEAR  y = act(x) . W^T + bias.  A lane adds at most 8 terms per 16-byte chunk it holds (the 8 products, the last of these
    additions into its accumulator), the 16 lanes of a column are joined in a 4-step exchange, the bias add is one more:
    D = 8 ceil(K / 128) + 4 + 1 counts every addition of a lane, where a single product passes through only 7 + (ceil(K / 128) - 1) + 5
    of them (the first accumulation adds to an exact zero) and its own rounding - <= D for every K, whether or not the compiler
    contracts products into fused multiply-adds (a contracted product does not round at all).  So
    |y - ref| <= gamma_D sum |w| |act(x)| + u |ref|, gamma_D = D u / (1 - D u).
    With SILU every activation carries its own error first: the rounded constant and product move exp2's argument by 2u |arg|
    (ln2 |arg| 2u on its result, weighted e / (1 + e)), 1 + e and the final product round once each, and the hardware exp2 / rcp line
    adds norm_ref.SILU_HW (the same two instructions, measured); a reciprocal below the normal range is flushed
    (x = -88): |x| 2^-126 absolute.  That activation error enters the sum weighted |w| (1 + gamma_D).
    An adaptive bound can pass anything: tests/test_elem_ref_cpu.py asserts bound <= 2^-10 (|ref| + 1) on every sweep input.
  * TIME_EMBEDDING  f = float32(10000 ** (-i / 160)), x = float32(f t), out = (cos, sin)(float64(x)) rounded once:
    u |ref| (1 + 2^-20) + 2^-149.  (No frequency lies within 2^-40 relative of a float32 rounding midpoint - asserted by the CPU test -
    so a last-place difference in the device's pow cannot move f.)
  * GEGLU_ERF  out = a 0.5 g (1 + erf(g / sqrt 2)), erf by Abramowitz-Stegun 7.1.26.  The fp32 error is absolute in the erf term:
    0.5 |a| |g| (1.5e-7 + c u).  c counts, in units of u on a term of magnitude <= 1 (<= 2 for 1 + erf): z = |g| 0.7071 and
    1 + 0.3275911 z: 3 roundings through t = rcp(.), |t poly'(t)| <= 1 -> 3; the five Horner steps, two roundings each on
    intermediates <= 1.5 in magnitude, each later multiplied by t <= 1 -> 15; exp2's argument -log2e z z: 3 roundings and twice z's
    2u -> 7u |arg| on the argument, ln2 arg exp(-z^2) <= ln2 / e on the result -> 3; poly exp2, 1 - ., 1 + copysign -> 1 + 1 + 2; the
    products 0.5 g (.) and a (.) -> 3 roundings relative to a term <= 2 -> 6; in all c = 31, plus the hardware rcp and exp2: SILU_HW
    each.  Then one fp16 rounding.
  * QUICK_GELU  f / (1 + exp(-1.702 f)) with __expf = the hardware exp2 of a rounded product: with s = 1 / (1 + e) the error of e moves
    the result by |f| s (1 - s) (relative error of e) - absolute in |f| where 1 + e cancels nothing but e is everything -; the argument
    carries 4 roundings (the constants 1.702 and log2 e and their two products: 4u |arg| on e), the hardware SILU_HW; 1 + e and the
    division round once each: 2u |ref|.  One fp16 rounding.  (The references use the exact constants 1.702, sqrt(2 / pi), 0.044715,
    0.18215 of the formulas: the float the kernel holds for each is one of the counted roundings.)
  * UNARY 0 (silu, library expf)  as QUICK_GELU with an exact argument and EXPF_LIB for the function.  UNARY 1 (gelu-tanh):
    w = 0.79788 (x + 0.044715 x^3) carries 7 roundings, |w tanh'(w)| <= 0.448 -> 3.2u on tanh, plus TANHF_ABS; 1 + tanh rounds
    once (<= 2u absolute): 0.5 |x| (5.2u + TANHF_ABS) + 2u |ref|, absolute in |x| where 1 + tanh cancels.  Both add 2^-118 for results
    below the normal range.  UNARY 2 (to-pixel): clamp((v + 1) 127.5, 0, 255) is two roundings before a 1-Lipschitz clamp:
    2u |(v + 1) 127.5| (1 + u); NaN -> 0, +-inf -> 255 / 0, each counted.
  * ENCODER_SAMPLE  (mean + noise sd) 0.18215, sd = sqrtf(expf(clamp(logvar, -30, 20))): the product with sd, the sum and the scale
    (rounded constant) round once each; sd carries SD_REL: 0.18215 (|noise| sd (SD_REL + 2u) + u (|mean| + |noise| sd)) + 2u |ref|.

The library functions' error is not derivable from IEEE rules; each constant below is 4x the largest value measured on an MI355X
against this module's float64 reference (the convention of tests/util.py; BASELINE.md section 4 names the input sets):
`function_error(d, ops, out)` is the measurement - the smallest constant with which the bound holds on a run's output.

`emulate` restates the device arithmetic in numpy, with seeded defects the check must reject.
"""
import math

import numpy as np

import replay
from norm_ref import SILU_HW, LOG2E32
from replay import NAN16, NAN32, f32_bits
from replay import bits_f32 as _f32

U32 = 2.0 ** -24
H16 = 2.0 ** -11
AS_ERF = 1.5e-7                     # stated maximum error of Abramowitz-Stegun 7.1.26
GEGLU_C = 31 * U32 + 2 * SILU_HW    # roundings of k_geglu_erf's erf term (module docstring) and its two hardware instructions
TINY = 2.0 ** -118                  # results below the fp32 normal range (an exponential that overflowed, a flushed quotient)
# Measured on an MI355X: the largest value `function_error` returns over the sweep case named - what the output
# needs beyond the derived roundings of its bound; allowed 4x.  Two of the three are zero: on those input sets the derived roundings
# alone cover every output of tanhf and of sqrtf(expf(.)), so their bounds are the derived part and nothing else.
EXPF_LIB_MEASURED = 0.369 * U32     # expf, relative: UNARY op 0, `unary_silu_grid` (90 013 fp32 inputs over [-100, 100])
TANHF_ABS_MEASURED = 0.0            # tanhf, absolute: UNARY op 1, `unary_gelu_grid` (the same inputs)
SD_REL_MEASURED = 0.0               # sqrtf(expf(.)), relative: ENCODER_SAMPLE, `encoder_sd_grid` (4096 log-variances over [-30, 20])
EXPF_LIB = 4 * EXPF_LIB_MEASURED
TANHF_ABS = 4 * TANHF_ABS_MEASURED
SD_REL = 4 * SD_REL_MEASURED


def _parse():
    txt = replay.header()
    return replay.enums(txt, {"TSD_ED_": "tsd_elem_desc_field", "TSD_EO_": "tsd_elem_operand", "TSD_EI_": "tsd_elem_info",
                              "TSD_EM_": "tsd_elem_mode"}) + [replay.version(txt, "TSD_ED_VERSION_1")]


ED, EO, EI, EM, ED_VERSION = _parse()
COUNT = ED["COUNT"]
INPUTS = ("X", "W", "BIAS")
OUTPUTS = ("Y",)
MODES = [k for k in EM if k != "COUNT"]
EXACT = ("CLIP_EMBED", "CHW_TO_NHWC", "IM2COL3X3", "NHWC_TO_CHW", "F32_TO_F16_ROWS", "F16_TO_F32_ROWS", "TRANSPOSE_TO_F16", "PACK_CONV",
         "PACK_LINEAR", "PACK_BIAS", "PACK_IM2COL_W")


FP16_STORE = ("GEGLU_ERF", "QUICK_GELU")   # arithmetic in fp32, one fp16 rounding at the store


# ---- descriptors ------------------------------------------------------------------------------------------------------------------
def desc(mode, **fields):
    d = np.zeros(COUNT, np.int64)
    d[ED["VERSION"]], d[ED["MODE"]] = ED_VERSION, EM[mode]
    for k, v in fields.items():
        d[ED[k.upper()]] = int(v)
    return d


def small_linear(B, K, N, ldx=None, ldw=None, ldy=None, silu=0, bias=1):
    return desc("SMALL_LINEAR", b=B, k=K, n=N, ldx=ldx or K, ldw=ldw or K, ldy=ldy or N, silu=silu, has_bias=bias)


def time_embedding(B, t=None):
    """t: the scalar every row uses; None: one t per row from the X operand."""
    return desc("TIME_EMBEDDING", b=B, has_t=int(t is None), t_bits=0 if t is None else f32_bits(t))


def geglu(rows, n_out):
    return desc("GEGLU_ERF", rows=rows, cols=n_out)


def quick_gelu(n):
    return desc("QUICK_GELU", n=n)


def unary(op, n):
    return desc("UNARY", op=op, n=n)


def clip_embed(B, T, V, D):
    return desc("CLIP_EMBED", b=B, t=T, v=V, d=D)


def chw_to_nhwc(B, C, H, W, cuse, cdst, scale=1.0):
    return desc("CHW_TO_NHWC", b=B, c=C, h=H, w=W, cuse=cuse, cdst=cdst, scale=f32_bits(scale))


def im2col(B, C, H, W, scale=1.0):
    return desc("IM2COL3X3", b=B, c=C, h=H, w=W, scale=f32_bits(scale))


def nhwc_to_chw(dtype, B, C, H, W, ld):
    """dtype 1: fp16 source, 0: fp32."""
    return desc("NHWC_TO_CHW", dtype=dtype, b=B, c=C, h=H, w=W, ld=ld)


def f32_to_f16_rows(rows, cols, ld, rows_dst):
    return desc("F32_TO_F16_ROWS", rows=rows, cols=cols, ld=ld, rows_dst=rows_dst)


def f16_to_f32_rows(rows, cols, ld):
    return desc("F16_TO_F32_ROWS", rows=rows, cols=cols, ld=ld)


def transpose_to_f16(B, K, N, Kpad, Npad):
    return desc("TRANSPOSE_TO_F16", b=B, k=K, n=N, kpad=Kpad, npad=Npad)


def pack_conv(O, I, k, Opad, Ipad):
    return desc("PACK_CONV", o=O, i=I, ksize=k, opad=Opad, ipad=Ipad)


def pack_linear(N, K, Kpad, interleave=0):
    return desc("PACK_LINEAR", n=N, k=K, kpad=Kpad, interleave=interleave)


def pack_bias(N, Npad, interleave=0):
    return desc("PACK_BIAS", n=N, npad=Npad, interleave=interleave)


def pack_im2col_w(O, Ipad, C):
    return desc("PACK_IM2COL_W", o=O, ipad=Ipad, c=C)


def encoder_sample(B, HW, ld):
    return desc("ENCODER_SAMPLE", b=B, hw=HW, ld=ld)


def F(d, k):
    return int(d[ED[k]])


def mode_of(d):
    return {v: k for k, v in EM.items()}[F(d, "MODE")]


def dtype_of(s, d):
    m = mode_of(d)
    h, f = np.float16, np.float32
    if m == "SMALL_LINEAR":
        return h if s == "W" else f
    if m in ("GEGLU_ERF", "QUICK_GELU", "PACK_IM2COL_W"):
        return h
    if m == "CLIP_EMBED":
        return {"X": np.int32, "W": h, "BIAS": f, "Y": h}[s]
    if m in ("CHW_TO_NHWC", "IM2COL3X3", "F32_TO_F16_ROWS", "TRANSPOSE_TO_F16", "PACK_CONV", "PACK_LINEAR"):
        return h if s == "Y" else f
    if m == "NHWC_TO_CHW":
        return h if s == "X" and F(d, "DTYPE") == 1 else f
    if m == "F16_TO_F32_ROWS":
        return f if s == "Y" else h
    return f


def extents(d):
    """Elements of every operand slot (0 = unused): what the entry's sizing-only mode must return."""
    e = dict.fromkeys(INPUTS + OUTPUTS, 0)
    m = mode_of(d)
    B, K, N, C, HW = F(d, "B"), F(d, "K"), F(d, "N"), F(d, "C"), F(d, "H") * F(d, "W")
    rows, cols, ld = F(d, "ROWS"), F(d, "COLS"), F(d, "LD")
    if m == "SMALL_LINEAR":
        e.update(X=(B - 1) * F(d, "LDX") + K, W=(N - 1) * F(d, "LDW") + K, BIAS=N if F(d, "HAS_BIAS") else 0, Y=(B - 1) * F(d, "LDY") + N)
    elif m == "TIME_EMBEDDING":
        e.update(X=B if F(d, "HAS_T") else 0, Y=B * 320)
    elif m == "GEGLU_ERF":
        e.update(X=rows * 2 * cols, Y=rows * cols)
    elif m in ("QUICK_GELU", "UNARY"):
        e.update(X=N, Y=N)
    elif m == "CLIP_EMBED":
        T, V, D = F(d, "T"), F(d, "V"), F(d, "D")
        e.update(X=B * T, W=V * D, BIAS=T * D, Y=B * T * D)
    elif m == "CHW_TO_NHWC":
        e.update(X=B * C * HW, Y=B * HW * F(d, "CDST"))
    elif m == "IM2COL3X3":
        e.update(X=B * C * HW, Y=B * HW * 64)
    elif m == "NHWC_TO_CHW":
        e.update(X=(B * HW - 1) * ld + C, Y=B * C * HW)
    elif m == "F32_TO_F16_ROWS":
        e.update(X=rows * cols, Y=F(d, "ROWS_DST") * ld)
    elif m == "F16_TO_F32_ROWS":
        e.update(X=(rows - 1) * ld + cols, Y=rows * cols)
    elif m == "TRANSPOSE_TO_F16":
        e.update(X=B * K * N, Y=B * F(d, "NPAD") * F(d, "KPAD"))
    elif m == "PACK_CONV":
        kk = F(d, "KSIZE") ** 2
        e.update(X=F(d, "O") * F(d, "I") * kk, Y=F(d, "OPAD") * kk * F(d, "IPAD"))
    elif m == "PACK_LINEAR":
        e.update(X=N * K, Y=N * F(d, "KPAD"))
    elif m == "PACK_BIAS":
        e.update(X=N, Y=F(d, "NPAD"))
    elif m == "PACK_IM2COL_W":
        e.update(X=F(d, "O") * 9 * F(d, "IPAD"), Y=F(d, "O") * 64)
    else:
        hw = F(d, "HW")
        e.update(X=(B * hw - 1) * ld + 8, W=B * 4 * hw, Y=B * 4 * hw)
    return e


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def pack(a2d, ld, dtype):
    """[rows][width] -> flat at pitch ld, the NaN fill in the pitch gaps."""
    rows, width = a2d.shape
    out = np.full((rows - 1) * ld + width, NAN16 if dtype == np.float16 else NAN32, dtype)
    out[(np.arange(rows)[:, None] * ld + np.arange(width)[None, :]).ravel()] = a2d.astype(dtype).ravel()
    return out


def unpack(flat, rows, width, ld):
    return flat[np.arange(rows)[:, None] * ld + np.arange(width)[None, :]]


def coded16(n, start=0):
    """n distinct fp16 values: element i is the (start + i)-th step of a fixed walk (stride 7919, coprime to the count) through the
    61 440 normal fp16 bit patterns, so neighbours in index are far apart in value and no two elements are equal."""
    i = (np.arange(start, start + n, dtype=np.int64) * 7919) % 61440
    assert n <= 61440
    return (0x0400 + (i % 30720) + np.where(i >= 30720, 0x8000, 0)).astype(np.uint16).view(np.float16)


# fp32 sources the conversions must round as numpy does: ties to even in the normal range, at the overflow threshold and at the bottom of
# the subnormal range; values beyond 65504; values that are subnormal in fp16
SPECIALS = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 65519.996, 65520.0, -65520.0, 1e5, -7e4, 2.0 ** -25, 3 * 2.0 ** -25,
                     -2.0 ** -25 * 1.0000001, 1e-7, -3.3e-6, 2.0 ** -14 - 2.0 ** -26, 5 * 2.0 ** -25, 0.0], np.float32)


def coded32(n, start=0, specials=True):
    x = coded16(n, start).astype(np.float32)
    if specials:
        k = min(len(SPECIALS), n // 3)
        x[(np.arange(k) * 3 + 1) % n] = SPECIALS[:k]
    return x


def all_f16(lim_bits=0x7C00):
    """Every fp16 of magnitude bits below lim_bits, both signs (0x7C00: all finite values, 63 488 of them)."""
    h = np.arange(lim_bits, dtype=np.uint16)
    return np.concatenate([h, h | 0x8000]).view(np.float16)


def unary_grid():
    """Dense fp32 inputs over [-100, 100] (finer over [-10, 10]) plus +-0, +-1e-30, +-1e30: 90 013 values."""
    g = np.concatenate([np.linspace(-100, 100, 50001), np.linspace(-10, 10, 40001), [0.0, -0.0, 1e-30, -1e-30, 1e30, -1e30, 1.0, -1.0, 0.5, -0.5, 20]])
    return g.astype(np.float32)


def make_inputs(d, seed=0, kind=None):
    """Seeded operands of descriptor d; `kind` selects a case's special inputs."""
    m = mode_of(d)
    r = np.random.default_rng(seed + 104729)
    e = extents(d)
    B, K, N, C, HW = F(d, "B"), F(d, "K"), F(d, "N"), F(d, "C"), F(d, "H") * F(d, "W")
    ops = {}
    if m == "SMALL_LINEAR":
        silu = F(d, "SILU")
        x = (r.standard_normal((B, K)) * (3 if silu else 1)).astype(np.float32)
        if kind == "silu_edges":
            x[:, :8] = np.array([20, -20, 88, -88, 0.0, -0.0, 1.0, -1.0], np.float32)
        w = r.uniform(-1, 1, (N, K)) / np.sqrt(K)
        if kind == "one_hot":      # measurement (K = N = 8): output column n is the activation of x[b][n] alone
            x = r.uniform(-20, 20, (B, K)).astype(np.float32)
            w = np.eye(N, K)
        ops["X"] = pack(x, F(d, "LDX"), np.float32)
        ops["W"] = pack(w, F(d, "LDW"), np.float16)
        if F(d, "HAS_BIAS"):
            ops["BIAS"] = (0.0 if kind == "one_hot" else 0.2) * r.standard_normal(N).astype(np.float32)
    elif m == "TIME_EMBEDDING":
        if F(d, "HAS_T"):
            ops["X"] = np.asarray(kind, np.float32)
            assert ops["X"].size == B
    elif m == "GEGLU_ERF":
        rows, n = F(d, "ROWS"), F(d, "COLS")
        if kind == "all_gates":        # every finite fp16 gate in [-8, 8] paired with a in {1, -3.5, 1000}; the tail is (1, 0) pairs
            g = all_f16(0x4801)
            a = np.repeat(np.array([1, -3.5, 1000], np.float16), g.size)
            g = np.tile(g, 3)
            pad = rows * n - g.size
            assert 0 <= pad < 8
            a, g = np.concatenate([a, np.ones(pad, np.float16)]), np.concatenate([g, np.zeros(pad, np.float16)])
        else:
            a, g = (2 * r.standard_normal(rows * n)).astype(np.float16), (2.5 * r.standard_normal(rows * n)).astype(np.float16)
        ops["X"] = np.stack([a, g], axis=1).ravel()
    elif m == "QUICK_GELU":
        ops["X"] = all_f16() if kind == "all_f16" else (3 * r.standard_normal(N)).astype(np.float16)
        assert ops["X"].size == N
    elif m == "UNARY":
        if kind == "grid":
            x = unary_grid()
        elif kind == "pixel":          # [-1.5, 1.5] with 3 NaN and 2 inf at known places
            x = np.linspace(-1.5, 1.5, N).astype(np.float32)
            x[[5, 700, N - 1]] = np.nan
            x[[6, 701]] = [np.inf, -np.inf]
        else:
            x = (3 * r.standard_normal(N)).astype(np.float32)
        assert x.size == N
        ops["X"] = x
    elif m == "CLIP_EMBED":
        T, V, D = F(d, "T"), F(d, "V"), F(d, "D")
        tok = r.integers(0, V, B * T).astype(np.int32)
        tok[:5] = [-5, 0, V - 1, V, 10 ** 6]
        ops["X"] = tok
        ops["W"] = coded16(V * D)
        pos = (coded16(T * D, start=V * D).astype(np.float32) * np.float32(0.37)).astype(np.float32)
        k = min(len(SPECIALS), T * D // 3)
        pos[(np.arange(k) * 3 + 1) % (T * D)] = SPECIALS[:k]
        ops["BIAS"] = pos
    elif m in ("CHW_TO_NHWC", "IM2COL3X3", "F32_TO_F16_ROWS", "TRANSPOSE_TO_F16", "PACK_CONV", "PACK_LINEAR"):
        ops["X"] = coded32(e["X"])
    elif m == "PACK_BIAS":
        ops["X"] = coded32(e["X"], specials=False) * np.float32(1.0001)   # fp32 -> fp32: values that are no fp16
    elif m == "PACK_IM2COL_W":
        ops["X"] = coded16(e["X"])
    elif m in ("NHWC_TO_CHW", "F16_TO_F32_ROWS"):
        if m == "NHWC_TO_CHW":
            rows, width, ld = B * HW, C, F(d, "LD")
        else:
            rows, width, ld = F(d, "ROWS"), F(d, "COLS"), F(d, "LD")
        dt = dtype_of("X", d)
        v = coded16(rows * width)
        v = v if dt == np.float16 else coded32(rows * width, specials=False) * np.float32(1.0001)
        v = v.copy()
        if kind and kind.startswith("nonfinite"):     # "nonfinite4": inf, -inf and two NaN at known places
            n = int(kind[len("nonfinite"):])
            bad = np.array([np.inf, -np.inf, np.nan, np.nan], dt)[:n] if n == 4 else np.array([np.inf, np.nan], dt)
            v[(np.arange(n) * 5 + 2) % v.size] = bad
        ops["X"] = pack(v.reshape(rows, width), ld, dt)
    else:   # ENCODER_SAMPLE
        hw, ld = F(d, "HW"), F(d, "LD")
        mom = np.zeros((B * hw, 8), np.float32)
        mom[:, :4] = r.standard_normal((B * hw, 4))
        mom[:, 4:] = r.uniform(-30, 20, (B * hw, 4))
        noise = r.standard_normal(B * 4 * hw).astype(np.float32)
        if kind == "sd_grid":          # measurement: mean 0, noise 1 -> out = 0.18215 sd over a dense grid of log-variances
            mom[:, :4] = 0
            mom[:, 4:] = np.linspace(-30, 20, B * hw * 4).reshape(B * hw, 4)
            noise[:] = 1
        else:
            mom[0, 4:7] = [-40, 30, 0]
            mom[1, 0] = np.nan          # one NaN mean
            mom[2, 5] = np.nan          # one NaN log-variance
        ops["X"] = pack(mom, ld, np.float32)
        ops["W"] = noise
    for s in INPUTS:
        assert (ops[s].size if s in ops else 0) == e[s], (m, s, e[s])
        if s in ops:
            ops[s] = np.ascontiguousarray(ops[s], dtype_of(s, d))
    return ops


# ---- references -----------------------------------------------------------------------------------------------------------------
def _gamma(n):
    return n * U32 / (1 - n * U32)


def silu64(x):
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def gelu_erf64(g):
    return 0.5 * g * (1.0 + np.vectorize(math.erf, otypes=[np.float64])(g / math.sqrt(2.0)))


def time_freqs():
    """(float64 10000 ** (-i / 160), its float32 rounding)."""
    f64 = 10000.0 ** (-np.arange(160, dtype=np.float64) / 160.0)
    return f64, f64.astype(np.float32)


def sl_operands(d, ops):
    B, K, N = F(d, "B"), F(d, "K"), F(d, "N")
    x = unpack(ops["X"], B, K, F(d, "LDX")).astype(np.float64)
    w = unpack(ops["W"], N, K, F(d, "LDW")).astype(np.float64)
    b = ops["BIAS"].astype(np.float64) if "BIAS" in ops else np.zeros(N)
    return x, w, b


def _sigmoid_terms(x, c):
    """s = 1 / (1 + exp(-c x)) and s (1 - s), in float64 without overflow."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp(-c * x)
        s = 1.0 / (1.0 + e)
        return s, np.where(np.isfinite(e), e / (1.0 + e) ** 2, 0.0)


def terms(d, ops):
    """(ref, base, weight): float64 reference in the output's logical shape, the derived part of the bound (for the modes that store fp16:
    of the fp32 value before the store), and the weight of the family's measured function-error constant (None where the bound has
    none): bound = base + weight * constant."""
    m = mode_of(d)
    if m == "SMALL_LINEAR":
        x, w, b = sl_operands(d, ops)
        K = F(d, "K")
        a, ea = x, np.zeros_like(x)
        if F(d, "SILU"):
            a = silu64(x)
            arg = np.abs(x) * LOG2E32
            s, _ = _sigmoid_terms(x, 1.0)
            rel = (2 * np.log(2.0) * arg * (1 - s) + 3) * U32 + SILU_HW
            ea = np.abs(a) * rel + np.abs(x) * 2.0 ** -126
        ref = a @ w.T + b
        D = 8 * -(-K // 128) + 4 + 1
        g = _gamma(D)
        base = g * (np.abs(a) @ np.abs(w).T) + U32 * np.abs(ref) + (1 + g) * (ea @ np.abs(w).T)
        return ref, base, None
    if m == "TIME_EMBEDDING":
        B = F(d, "B")
        t = ops["X"] if F(d, "HAS_T") else np.full(B, _f32(F(d, "T_BITS")), np.float32)
        _, f = time_freqs()
        x = (f[None, :] * t.astype(np.float32)[:, None]).astype(np.float32).astype(np.float64)
        ref = np.concatenate([np.cos(x), np.sin(x)], axis=1)
        return ref, U32 * np.abs(ref) * (1 + 2.0 ** -20) + 2.0 ** -149, None
    if m == "GEGLU_ERF":
        v = ops["X"].astype(np.float64).reshape(F(d, "ROWS"), F(d, "COLS"), 2)
        a, g = v[..., 0], v[..., 1]
        ref = a * gelu_erf64(g)
        e32 = 0.5 * np.abs(a) * np.abs(g) * (AS_ERF + GEGLU_C)
        return ref, e32, None
    if m == "QUICK_GELU":
        f = ops["X"].astype(np.float64)
        c = 1.702
        s, s1s = _sigmoid_terms(f, c)
        ref = f * s
        e32 = np.abs(f) * s1s * (4 * U32 * np.abs(c * f) + SILU_HW) + 2 * U32 * np.abs(ref) + TINY
        return ref, e32, None
    if m == "UNARY":
        x = ops["X"].astype(np.float64)
        op = F(d, "OP")
        if op == 0:
            s, s1s = _sigmoid_terms(x, 1.0)
            ref = x * s
            return ref, 2 * U32 * np.abs(ref) + TINY, np.abs(x) * s1s
        if op == 1:
            with np.errstate(over="ignore"):
                w = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)
            ref = 0.5 * x * (1.0 + np.tanh(w))
            return ref, 0.5 * np.abs(x) * 5.2 * U32 + 2 * U32 * np.abs(ref) + TINY, 0.5 * np.abs(x)
        pre = (x + 1.0) * 127.5
        ref = np.where(np.isnan(pre), 0.0, np.clip(pre, 0.0, 255.0))
        bd = np.where(np.isfinite(pre), 2 * U32 * np.abs(pre) * (1 + U32), 0.0)
        return ref, bd, None
    if m == "ENCODER_SAMPLE":
        B, hw, ld = F(d, "B"), F(d, "HW"), F(d, "LD")
        mom = unpack(ops["X"], B * hw, 8, ld).astype(np.float64).reshape(B, hw, 8)
        mean, lv = mom[..., :4].transpose(0, 2, 1), mom[..., 4:].transpose(0, 2, 1)          # [B][4][HW]
        lv = np.clip(np.where(np.isnan(lv), -30.0, lv), -30.0, 20.0)                          # fmaxf(NaN, -30) = -30
        sd = np.sqrt(np.exp(lv))
        nz = ops["W"].astype(np.float64).reshape(B, 4, hw)
        c = 0.18215
        ref = (mean + nz * sd) * c
        base = c * (2 * U32 * np.abs(nz) * sd + U32 * (np.abs(mean) + np.abs(nz) * sd)) + 2 * U32 * np.abs(ref)
        return ref, base, c * np.abs(nz) * sd
    raise ValueError(m)


def _constant(d):
    m = mode_of(d)
    if m == "UNARY":
        return (EXPF_LIB, TANHF_ABS, 0.0)[F(d, "OP")]
    return SD_REL if m == "ENCODER_SAMPLE" else 0.0


def reference(d, ops):
    """(ref64, bound) in the output's logical shape (arithmetic modes)."""
    ref, base, weight = terms(d, ops)
    if mode_of(d) in FP16_STORE:
        return ref, H16 * np.abs(ref) + (1 + H16) * base + 2.0 ** -25
    return ref, base if weight is None else base + weight * _constant(d)


def logical(d, out):
    """The output's logical elements, in the shape `reference` uses."""
    m = mode_of(d)
    if m == "SMALL_LINEAR":
        return unpack(out, F(d, "B"), F(d, "N"), F(d, "LDY"))
    if m == "TIME_EMBEDDING":
        return out.reshape(F(d, "B"), 320)
    if m == "GEGLU_ERF":
        return out.reshape(F(d, "ROWS"), F(d, "COLS"))
    if m == "ENCODER_SAMPLE":
        return out.reshape(F(d, "B"), 4, F(d, "HW"))
    return out


def function_error(d, ops, out):
    """The measurement: the smallest function-error constant with which the bound holds on this output (UNARY 0 / 1, ENCODER_SAMPLE)."""
    ref, base, weight = terms(d, ops)
    err = np.abs(logical(d, out).astype(np.float64) - ref)
    ok = np.isfinite(ref) & (weight > 2.0 ** -100)
    return float(np.max(np.where(ok, np.maximum(err - base, 0.0) / np.where(ok, weight, 1.0), 0.0)))


def _rne16(x32):
    with np.errstate(over="ignore"):
        return x32.astype(np.float16)


def expected(d, ops, mut=None):
    """The movement modes: the exact output, every element (flat, in the output's type).  `mut` seeds one defect."""
    m = mode_of(d)
    B, K, N, C, H, W = F(d, "B"), F(d, "K"), F(d, "N"), F(d, "C"), F(d, "H"), F(d, "W")
    HW = H * W
    x = ops["X"]
    if m == "CLIP_EMBED":
        T, V, D = F(d, "T"), F(d, "V"), F(d, "D")
        tok = np.clip(x.astype(np.int64), 0, V - 1)
        row = np.arange(B * T)
        p = (row // T) if mut == "pos_row_div" else (row % T)
        return _rne16(ops["W"].reshape(V, D)[tok].astype(np.float32) + ops["BIAS"].reshape(T, D)[p]).ravel()
    scale = np.float32(_f32(F(d, "SCALE")))
    if m == "CHW_TO_NHWC":
        cuse, cdst = F(d, "CUSE"), F(d, "CDST")
        y = np.zeros((B, HW, cdst), np.float16)
        n = min(cuse, cdst)
        y[:, :, :n] = _rne16(x.reshape(B, C, HW)[:, :n] * scale).transpose(0, 2, 1)
        return y.ravel()
    if m == "IM2COL3X3":
        xs = _rne16(x.reshape(B, C, H, W) * scale)
        y = np.zeros((B, H, W, 64), np.float16)
        for t in range(9):
            dy, dx = (t % 3 - 1, t // 3 - 1) if mut == "tap_transposed" else (t // 3 - 1, t % 3 - 1)
            for yy in range(H):
                for xx in range(W):
                    iy, ix = yy + dy, xx + dx
                    wlim = W - 1 if mut == "edge_off_by_one" else W
                    if 0 <= iy < H and 0 <= ix < wlim:
                        y[:, yy, xx, t * C:(t + 1) * C] = xs[:, :, iy, ix]
        return y.ravel()
    if m == "NHWC_TO_CHW":
        return unpack(x, B * HW, C, F(d, "LD")).reshape(B, HW, C).transpose(0, 2, 1).astype(np.float32).ravel()
    if m == "F32_TO_F16_ROWS":
        rows, cols = F(d, "ROWS"), F(d, "COLS")
        y = np.zeros((F(d, "ROWS_DST"), F(d, "LD")), np.float16)
        y[:rows, :cols] = _rne16(x.reshape(rows, cols))
        return y.ravel()
    if m == "F16_TO_F32_ROWS":
        return unpack(x, F(d, "ROWS"), F(d, "COLS"), F(d, "LD")).astype(np.float32).ravel()
    if m == "TRANSPOSE_TO_F16":
        y = np.zeros((B, F(d, "NPAD"), F(d, "KPAD")), np.float16)
        y[:, :N, :K] = _rne16(x.reshape(B, K, N)).transpose(0, 2, 1)
        return y.ravel()
    if m == "PACK_CONV":
        O, I, k = F(d, "O"), F(d, "I"), F(d, "KSIZE")
        y = np.zeros((F(d, "OPAD"), k * k, F(d, "IPAD")), np.float16)
        y[:O, :, :I] = _rne16(x.reshape(O, I, k * k)).transpose(0, 2, 1)
        if mut == "tap_channel_swapped":   # channel-major: K index = channel * taps + tap
            y = np.ascontiguousarray(y.transpose(0, 2, 1))
        return y.ravel()
    if m in ("PACK_LINEAR", "PACK_BIAS"):
        r = np.arange(N)
        sr = r
        if F(d, "INTERLEAVE"):
            sr = np.where(r & 1, N // 2 + (r >> 1), r >> 1)
            if mut == "halves_swapped":
                sr = np.where(r & 1, r >> 1, N // 2 + (r >> 1))
        if m == "PACK_BIAS":
            y = np.zeros(F(d, "NPAD"), np.float32)
            y[:N] = x[sr]
            return y
        y = np.zeros((N, F(d, "KPAD")), np.float16)
        y[:, :K] = _rne16(x.reshape(N, K)[sr])
        return y.ravel()
    if m == "PACK_IM2COL_W":
        O, ipad = F(d, "O"), F(d, "IPAD")
        y = np.zeros((O, 64), np.float16)
        y[:, :9 * C] = x.reshape(O, 9, ipad)[:, :, :C].reshape(O, 9 * C)
        return y.ravel()
    raise ValueError(m)


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def check(d, ops, out, info=None):
    """out: the flat device (or emulated) Y.  Returns (failures, worst error / bound): movement modes compare bit patterns (0 or inf)."""
    m = mode_of(d)
    fails = []
    if m in EXACT:
        want = expected(d, ops)
        if out.dtype != want.dtype or out.shape != want.shape:
            return [f"output {out.dtype}{out.shape}, expected {want.dtype}{want.shape}"], np.inf
        bad = _bits(out) != _bits(want)
        if bad.any():
            i = int(np.argmax(bad))
            fails.append(f"{int(bad.sum())} of {bad.size} elements differ in their bits, first at {i}: got {out[i]!r} "
                         f"({int(_bits(out)[i]):#x}) expected {want[i]!r} ({int(_bits(want)[i]):#x})")
        return fails, np.inf if fails else 0.0
    ref, bd = reference(d, ops)
    got = logical(d, out).astype(np.float64)
    nan_ok = np.isnan(ref) & np.isnan(got)            # a NaN mean stays a NaN (ENCODER_SAMPLE)
    err = np.where(nan_ok, 0.0, np.abs(got - ref))
    bad = ~(err <= bd) & ~nan_ok
    ratio = float(np.max(np.where(np.isfinite(err), err, np.inf) / np.where(nan_ok, 1.0, np.maximum(bd, 1e-300))))
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, np.where(np.isfinite(err), err / np.maximum(bd, 1e-300), np.inf), 0))), err.shape)
        fails.append(f"{int(bad.sum())} of {bad.size} elements outside the bound, worst at {tuple(int(v) for v in i)}: got {got[i]!r} "
                     f"ref {ref[i]!r} err {err[i]:.3e} bound {bd[i]:.3e}")
    if m == "SMALL_LINEAR":                           # the pitch gaps of y still hold the fill
        gap = np.ones(out.size, bool)
        gap[(np.arange(F(d, "B"))[:, None] * F(d, "LDY") + np.arange(F(d, "N"))[None, :]).ravel()] = False
        if (out.view(np.uint32)[gap] != NAN32.view(np.uint32)).any():
            fails.append("a pitch gap of y was written")
            ratio = np.inf
    return fails, ratio


def fp32_share(d, ops):
    """The bound without its fp16 rounding (the modes that store fp16): what the fp32 value before the store is held to."""
    assert mode_of(d) in FP16_STORE
    return terms(d, ops)[:2]


def cap_violations(d, ops):
    """SMALL_LINEAR: elements whose bound exceeds 2^-10 (|ref| + 1), and the largest bound / cap."""
    ref, bd = reference(d, ops)
    cap = 2.0 ** -10 * (np.abs(ref) + 1)
    return int((bd > cap).sum()), float((bd / cap).max())


# ---- numpy emulation of the device arithmetic -----------------------------------------------------------------------------------------
def _silu_hw32(f):
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2(np.float32(-1.4426950408889634) * f).astype(np.float32)
        return (f * (np.float32(1) / (np.float32(1) + e))).astype(np.float32)


def _emulate_small_linear(d, ops, mut):
    B, K, N, ldy = F(d, "B"), F(d, "K"), F(d, "N"), F(d, "LDY")
    x = unpack(ops["X"], B, K, F(d, "LDX")).astype(np.float32)
    w = unpack(ops["W"], N, K, F(d, "LDW")).astype(np.float32)
    if F(d, "SILU") and mut != "no_silu":
        x = _silu_hw32(x)
    nchunk = -(-K // 128) * 16                                       # 16-byte chunks, padded to whole rows of 16 lanes
    xp, wp = np.zeros((B, nchunk * 8), np.float32), np.zeros((N, nchunk * 8), np.float32)
    xp[:, :K], wp[:, :K] = x, w
    if mut == "last_chunk":                                          # the lane that holds the last chunk drops it
        wp[:, K - 8:K] = 0
    if mut == "second_pass":
        wp[:, 2048:] = 0
    p = wp.reshape(1, N, nchunk // 16, 16, 8) * xp.reshape(B, 1, nchunk // 16, 16, 8)      # [B][N][it][lane][8]
    acc = np.zeros((B, N, 16), np.float32)
    for it in range(nchunk // 16):
        s = p[:, :, it, :, 0]
        for j in range(1, 8):
            s = s + p[:, :, it, :, j]
        acc = acc + s
    o = 8
    while o:
        acc = acc + acc[:, :, np.arange(16) ^ o]
        o //= 2
    y = acc[:, :, 0]
    if "BIAS" in ops:
        b = ops["BIAS"]
        y = y + (np.roll(b, -1) if mut == "bias_col" else b)
    if mut == "b_nb":
        y = y.copy()
        y[B - 1] = y[0]
    out = pack(y, ldy, np.float32)
    if mut == "row_clamp":                                           # no store mask: columns N .. of the block get row N - 1's result
        for b in range(B):
            for n in range(N, -(-N // 16) * 16):
                if b * ldy + n < out.size:
                    out[b * ldy + n] = y[b, N - 1]
    return out


def emulate(d, ops, mut=None, raw=False):
    """The device arithmetic restated in numpy: flat Y as the device lays it out.  `mut` seeds one defect; raw: the fp32 values before an
    fp16 store, in the logical shape."""
    m = mode_of(d)
    if m in EXACT:
        return expected(d, ops, mut)
    f32 = np.float32
    if m == "SMALL_LINEAR":
        return _emulate_small_linear(d, ops, mut)
    if m == "TIME_EMBEDDING":
        B = F(d, "B")
        t = ops["X"] if F(d, "HAS_T") else np.full(B, _f32(F(d, "T_BITS")), f32)
        if mut == "row_t0":
            t = np.full(B, t[0], f32)
        x = (time_freqs()[1][None, :] * t.astype(f32)[:, None]).astype(f32).astype(np.float64)
        halves = [np.sin(x), np.cos(x)] if mut == "sincos_swapped" else [np.cos(x), np.sin(x)]
        return np.concatenate(halves, axis=1).astype(f32).ravel()
    if m == "GEGLU_ERF":
        v = ops["X"].astype(f32).reshape(-1, 2)
        a, g = (v[:, 1], v[:, 0]) if mut == "swap_a_gate" else (v[:, 0], v[:, 1])
        if mut == "tanh_gelu":
            gl = f32(0.5) * g * (f32(1) + np.tanh(f32(0.7978845608028654) * (g + f32(0.044715) * g * g * g)))
        else:
            z = np.abs(g) * f32(0.7071067811865476)
            t = f32(1) / (f32(1) + f32(0.3275911) * z)
            poly = t * (f32(0.254829592) + t * (f32(-0.284496736) + t * (f32(1.421413741) + t * (f32(-1.453152027) + t * f32(1.061405429)))))
            with np.errstate(under="ignore"):
                er = f32(1) - poly * np.exp2(f32(-1.4426950408889634) * z * z).astype(f32)
            gl = f32(0.5) * g * (f32(1) + np.copysign(er, g))
        y = (a * gl).astype(f32)
        return y.reshape(F(d, "ROWS"), F(d, "COLS")) if raw else _rne16(y)
    if m == "QUICK_GELU":
        f = ops["X"].astype(f32)
        with np.errstate(over="ignore", under="ignore"):
            y = (f / (f32(1) + np.exp2(f32(1.4426950408889634) * (f32(-1.702) * f)).astype(f32))).astype(f32)
        return y if raw else _rne16(y)
    if m == "UNARY":
        x, op = ops["X"], F(d, "OP")
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            if op == 0:    # a correctly rounded expf
                return (x / (f32(1) + np.exp(-x.astype(np.float64)).astype(f32))).astype(f32)
            if op == 1:
                return (f32(0.5) * x * (f32(1) + np.tanh(f32(0.7978845608028654) * (x + f32(0.044715) * x * x * x)))).astype(f32)
            pre = (x + f32(1)) * f32(127.5)
            return np.where(np.isnan(pre), f32(0), np.clip(pre, f32(0), f32(255))).astype(f32)
    B, hw = F(d, "B"), F(d, "HW")
    mom = unpack(ops["X"], B * hw, 8, F(d, "LD")).reshape(B, hw, 8)
    mean, lv = mom[..., :4].transpose(0, 2, 1), mom[..., 4:].transpose(0, 2, 1)
    lv = np.clip(np.where(np.isnan(lv), f32(-30), lv), f32(-30), f32(20))
    sd = np.sqrt(np.exp(lv).astype(f32)).astype(f32)
    return ((mean + ops["W"].reshape(B, 4, hw) * sd) * f32(0.18215)).astype(f32).ravel()


def nonfinite_expected(d, ops):
    """What the kernels that count non-finite values must report for these operands."""
    m = mode_of(d)
    if m == "NHWC_TO_CHW":
        return int((~np.isfinite(unpack(ops["X"], F(d, "B") * F(d, "H") * F(d, "W"), F(d, "C"), F(d, "LD")).astype(np.float32))).sum())
    if m == "F16_TO_F32_ROWS":
        return int((~np.isfinite(unpack(ops["X"], F(d, "ROWS"), F(d, "COLS"), F(d, "LD")).astype(np.float32))).sum())
    if m == "UNARY" and F(d, "OP") == 2:
        return int((~np.isfinite(ops["X"])).sum())
    if m == "ENCODER_SAMPLE":
        return int((~np.isfinite(unpack(ops["X"], F(d, "B") * F(d, "HW"), 8, F(d, "LD")))).sum())
    return 0


# ---- the sweep: (name, descriptor, input kind, expected info fields) -----------------------------------------------------------------
T16 = [0, 999, 0.5, 1, 20, 980, 333.25, 7, 42, 100, 250, 500, 640, 777, 901, 998]


def _nb(B):
    return 1 if B <= 1 else 2 if B <= 2 else 4 if B <= 4 else 8 if B <= 8 else 16


def _sl(name, B, K, N, kind=None, **kw):
    return (name, small_linear(B, K, N, **kw), kind, dict(NB=_nb(B), PASSES=-(-K // 2048), NONFINITE=0))


def sweep():
    S = []
    nf0 = dict(NONFINITE=0)
    # SMALL_LINEAR: every NB instance full and partly filled
    for B in (1, 2, 3, 4, 5, 8, 9, 16):
        for silu in (0, 1):
            S.append(_sl(f"sl_b{B}_k320_n48_silu{silu}", B, 320, 48, silu=silu))
    # K: one live lane, a ragged chunk row, the second `it`, one pass exactly, the second pass
    for K in (8, 120, 128, 136, 1288, 2048, 2056, 2560):
        for silu in (0, 1):
            S.append(_sl(f"sl_k{K}_b3_n17_silu{silu}", 3, K, 17, silu=silu))
    for N in (1, 15, 16, 17, 33):
        S.append(_sl(f"sl_n{N}_b2_k128", 2, 128, N))
    for silu in (0, 1):
        S.append(_sl(f"sl_pitches_silu{silu}", 3, 136, 17, ldx=140, ldw=144, ldy=20, silu=silu))
    S.append(_sl("sl_pitches_k2056", 5, 2056, 33, ldx=2060, ldw=2064, ldy=36, silu=1))
    S.append(_sl("sl_lds_160k", 16, 2560, 16, silu=1))
    S.append(_sl("sl_prod_320_1280", 16, 320, 320, silu=0))
    S.append(_sl("sl_prod_1280_1280", 16, 1280, 320, silu=1))
    S.append(_sl("sl_prod_1280_n", 16, 1280, 320, silu=1, ldy=328))
    S.append(_sl("sl_no_bias", 3, 320, 48, bias=0))
    S.append(_sl("sl_no_bias_silu", 3, 320, 48, bias=0, silu=1))
    S.append(_sl("sl_silu_edges", 4, 320, 48, kind="silu_edges", silu=1))
    # TIME_EMBEDDING
    for t in (0, 1, 20, 980, 999):
        for B in (1, 3):
            S.append((f"temb_t{t}_b{B}", time_embedding(B, float(t)), None, nf0))
    S.append(("temb_array_b16", time_embedding(16), T16, nf0))
    S.append(("temb_array_b1", time_embedding(1), [980.0], nf0))
    # GEGLU_ERF
    S.append(("geglu_all_gates", geglu(50, 2212), "all_gates", nf0))
    S.append(("geglu_random", geglu(3, 20), None, nf0))
    # QUICK_GELU
    S.append(("quick_gelu_all_f16", quick_gelu(63488), "all_f16", nf0))
    # UNARY
    ng = unary_grid().size
    S.append(("unary_silu_grid", unary(0, ng), "grid", nf0))
    S.append(("unary_gelu_grid", unary(1, ng), "grid", nf0))
    S.append(("unary_pixel", unary(2, 4001), "pixel", dict(NONFINITE=5)))
    # CLIP_EMBED
    for D in (8, 768, 1032):
        S.append((f"clip_d{D}", clip_embed(3, 5, 11, D), None, nf0))
    # layout conversions
    for C in (1, 3, 4, 7):
        for (H, W) in ((1, 1), (2, 5), (5, 3), (8, 8)):
            for B in (1, 3):
                for sc, sn in ((1.0, "1"), (1 / 0.18215, "vae")):
                    S.append((f"im2col_c{C}_{H}x{W}_b{B}_s{sn}", im2col(B, C, H, W, sc), None, nf0))
    for (C, cuse, cdst) in ((4, 4, 8), (5, 3, 8), (12, 12, 16), (8, 8, 24)):
        for sc, sn in ((1.0, "1"), (1 / 0.18215, "vae")):
            S.append((f"nhwc_c{C}_use{cuse}_dst{cdst}_s{sn}", chw_to_nhwc(2, C, 3, 5, cuse, cdst, sc), None, nf0))
    for dt in (1, 0):
        S.append((f"chw_from_{'f16' if dt else 'f32'}", nhwc_to_chw(dt, 2, 5, 2, 3, 8), None, nf0))
        S.append((f"chw_from_{'f16' if dt else 'f32'}_nonfinite", nhwc_to_chw(dt, 2, 5, 2, 3, 8), "nonfinite4", dict(NONFINITE=4)))
    S.append(("rows_f32_to_f16", f32_to_f16_rows(3, 5, 8, 4), None, nf0))
    S.append(("rows_f16_to_f32", f16_to_f32_rows(3, 5, 8), None, nf0))
    S.append(("rows_f16_to_f32_nonfinite", f16_to_f32_rows(3, 5, 8), "nonfinite2", dict(NONFINITE=2)))
    S.append(("transpose", transpose_to_f16(2, 5, 3, 8, 4), None, nf0))
    # packers
    for k in (1, 3):
        S.append((f"pack_conv_k{k}", pack_conv(3, 5, k, 4, 8), None, nf0))
    for il in (0, 1):
        S.append((f"pack_linear_il{il}", pack_linear(6, 5, 8, il), None, nf0))
        S.append((f"pack_bias_il{il}", pack_bias(6, 8, il), None, nf0))
    for C in (3, 4, 7):
        S.append((f"pack_im2col_w_c{C}", pack_im2col_w(3, 8, C), None, nf0))
    # ENCODER_SAMPLE
    for ld in (8, 12):
        S.append((f"encoder_ld{ld}", encoder_sample(2, 6, ld), None, dict(NONFINITE=2)))
    S.append(("encoder_sd_grid", encoder_sample(2, 512, 8), "sd_grid", nf0))
    return S


def refusals():
    """Launches the launchers refuse on the host: (name, descriptor)."""
    return [
        ("sl_b17", small_linear(17, 320, 48)),
        ("sl_k12", small_linear(3, 12, 17)),
        ("sl_ldx_k_plus_2", small_linear(3, 136, 17, ldx=138)),
        ("sl_lds_over", small_linear(16, 2568, 16)),
        ("geglu_n6", geglu(3, 6)),
        ("quick_gelu_n12", quick_gelu(12)),
        ("im2col_c8", im2col(1, 8, 2, 5)),
        ("nhwc_cdst12", chw_to_nhwc(2, 12, 3, 5, 12, 12)),
    ]


SWEEP = sweep()
