"""Reference of the FP8 feed-forward (csrc/kernels_fp8.hip, include/tsd.h "FP8 feed-forward"): the OCP e4m3 decode table in float64, the row
quantiser restated in numpy fp32 exactly as specified (bit for bit what the kernel must give), and a fake-quant linear - quantise, decode,
float64 matmul, epilogue in float64 - with the error bound of the GEMM.

The bound follows tests/gemm_ref.py, u = 2^-24: products of two e4m3 values are exact in fp32; the Kp-long fp32 accumulation loses at most
2 Kp u of sum|a||w| (the matrix core's adds may truncate); the two scale multiplies add 2 u; every epilogue add rounds once; GEGLU
propagates the two columns' errors through |gelu'| < 1.13 plus gelu_tanh_f's own (6 + 4 |arg|) u; the fp16 store adds 2^-11 of the value
plus 2^-25 in the subnormal range."""
import numpy as np

U32 = 2.0 ** -24
GELU_DMAX = 1.13
E4M3_MAX = np.float32(448.0)
EPI_NONE, EPI_GEGLU = 0, 1


def _decode_table():
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    v[(e == 15) & (m == 7)] = np.nan
    return np.where(c & 128, -v, v)


E4M3 = _decode_table()   # float64 [256]; codes 0x7f / 0xff are NaN


def e4m3_encode(v):
    """float32 values in [-448, 448] -> e4m3 bytes, round to nearest even (exact: every step is a power-of-two scaling or rint)."""
    v = np.asarray(v, np.float32)
    a = np.abs(v).astype(np.float64)
    _, ex = np.frexp(a)                      # a = f 2^ex, f in [0.5, 1)
    e = np.where(a < 2.0 ** -6, -6, ex - 1)  # exponent of the binade; the subnormal range (and zero) shares -6
    q = np.rint(a * 2.0 ** (3 - e)).astype(np.int64)   # multiples of 2^(e - 3): 8 .. 16 in a binade, 0 .. 8 below 2^-6
    code = np.where(e == -6, q, ((e + 7) << 3) + q - 8)   # q = 16 carries into the next binade, q = 8 below 2^-6 is the first normal
    return (code | np.where(np.signbit(v), 128, 0)).astype(np.uint8)


def quant_rows(x, K=None):
    """x float16 (M, ld) -> (q uint8 (M, Kp), scale float32 (M,)): the kernel's arithmetic in numpy fp32."""
    x = np.asarray(x, np.float16)
    M, ld = x.shape
    K = ld if K is None else K
    Kp = -(-K // 128) * 128
    xf = x[:, :K].astype(np.float32)
    amax = np.abs(xf).max(axis=1)
    bad = ~np.isfinite(xf).all(axis=1)
    flat = bad | (amax == 0)
    with np.errstate(all="ignore"):
        scale = np.where(bad, np.float32(np.nan), np.where(amax == 0, np.float32(1), amax / E4M3_MAX)).astype(np.float32)
        inv = np.where(flat, np.float32(0), E4M3_MAX / amax).astype(np.float32)
        y = np.clip(np.where(bad[:, None], np.float32(0), xf * inv[:, None]), -E4M3_MAX, E4M3_MAX)
    q = np.zeros((M, Kp), np.uint8)
    q[:, :K] = np.where(bad[:, None], 0, e4m3_encode(y))
    return q, scale


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def gemm(a8, sa, w8, sw, bias=None, residual=None, epi=EPI_NONE):
    """-> (ref float64, bound float64) of out[m][n] = rn16(epi(sa[m] sw[n] sum_k a8[m][k] w8[n][k])) over the decoded bytes."""
    A, W = E4M3[a8], E4M3[w8]
    s = np.asarray(sa, np.float64)[:, None] * np.asarray(sw, np.float64)[None, :]
    v, mag = s * (A @ W.T), np.abs(s) * (np.abs(A) @ np.abs(W).T)
    e = (2 * a8.shape[1] + 2) * U32 * mag
    terms = 0
    for t in (None if bias is None else np.asarray(bias, np.float64)[None, :], None if residual is None else np.asarray(residual, np.float64)):
        if t is not None:
            v, mag, terms = v + t, mag + np.abs(t), terms + 1
    e = e + (terms + 1) * U32 * mag
    if epi == EPI_GEGLU:
        a, g, ea, eg = v[:, 0::2], v[:, 1::2], e[:, 0::2], e[:, 1::2]
        gl = gelu_tanh64(g)
        arg = np.abs(np.sqrt(2.0 / np.pi) * 2.0 * np.log2(np.e) * (g + 0.044715 * g ** 3))
        v = a * gl
        e = np.abs(gl) * ea + (np.abs(a) + ea) * GELU_DMAX * eg + np.abs(v) * (6.0 + 4.0 * arg) * U32
    return v, 2.0 ** -11 * np.abs(v) + (1.0 + 2.0 ** -11) * e + 2.0 ** -25


def fake_quant_linear(x, w, bias=None):
    """x (M, K), w (N, K) -> float64 (M, N): both rounded to fp16 and quantised per row as the device does, decoded, multiplied in
    float64.  What the model-level reference puts in place of the two feed-forward linears."""
    (qx, sx), (qw, sw) = quant_rows(np.asarray(x, np.float16)), quant_rows(np.asarray(w, np.float16))
    y = (E4M3[qx] * sx[:, None].astype(np.float64)) @ (E4M3[qw] * sw[:, None].astype(np.float64)).T
    return y if bias is None else y + np.asarray(bias, np.float64)[None, :]
