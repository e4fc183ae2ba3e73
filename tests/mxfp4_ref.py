"""Reference of the MXFP4 weights of the opt-in 8-bit feed-forward (csrc/kernels_fp8.hip, include/tsd.h "MXFP4 weights"): the OCP MX v1.0
quantiser restated in numpy - bit for bit what k_quant_weights_mxfp4 must give in its plain row-major form - a dequantiser, and the W4A8
GEMM in float64 with its bound.

The bound is tests/fp8_ref.py's with the per-channel scale gone: an e4m3 value times an e2m1 value times a power of two is exact in fp32;
the Kp-long fp32 accumulation loses at most 2 Kp u of sum|a||w|; the one scale multiply adds u; the epilogue and the fp16 store as there."""
import numpy as np

import fp8_ref as R8

E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])   # float64 [16]: code = sign << 3 | magnitude code
MIDPOINTS = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])                        # between neighbouring magnitudes
E8M0_ONE = 127


def e2m1_encode(v):
    """float values -> e2m1 codes: nearest, a midpoint to the even code, beyond 6 saturating; the sign bit is the value's."""
    a = np.abs(np.asarray(v, np.float64))
    up = [a > 0.25, a >= 0.75, a > 1.25, a >= 1.75, a > 2.5, a >= 3.5, a > 5.0]   # ties 0.25, 1.25, 2.5, 5 stay; 0.75, 1.75, 3.5 go up
    return (np.sum(up, axis=0) | np.where(np.signbit(v), 8, 0)).astype(np.uint8)


def quant_weights(w, K=None):
    """w float16 (N, ld), K a multiple of 32 -> (elems uint8 (N, Kp / 2), scales uint8 (N, Kp / 32)), Kp = K rounded up to 128; raises
    FloatingPointError on a non-finite weight."""
    w = np.asarray(w, np.float16)
    N, ld = w.shape
    K = ld if K is None else K
    Kp = -(-K // 128) * 128
    blocks = w[:, :K].astype(np.float64).reshape(N, K // 32, 32)
    if not np.isfinite(blocks).all():
        raise FloatingPointError("non-finite weight")
    amax = np.abs(blocks).max(axis=2)
    ex = np.frexp(amax)[1] - 1                            # floor(log2 amax) where amax > 0
    byte = np.where(amax == 0, E8M0_ONE, ex - 2 + 127)
    codes = np.where((amax == 0)[:, :, None], 0, e2m1_encode(blocks * 2.0 ** -(byte - 127.0)[:, :, None]))
    full = np.zeros((N, Kp), np.uint8)
    full[:, :K] = codes.reshape(N, K)
    scales = np.full((N, Kp // 32), E8M0_ONE, np.uint8)
    scales[:, :K // 32] = byte
    return full[:, 0::2] | (full[:, 1::2] << 4), scales


def dequant(elems, scales):
    """-> float64 (N, Kp)"""
    codes = np.stack([elems & 15, elems >> 4], axis=2).reshape(elems.shape[0], -1)
    return E2M1[codes] * np.repeat(2.0 ** (scales.astype(np.float64) - 127), 32, axis=1)


def gemm(a8, sa, elems, scales, bias=None, residual=None, epi=R8.EPI_NONE):
    """-> (ref float64, bound float64) of out[m][n] = rn16(epi(sa[m] sum_k a8[m][k] X[n][k / 32] w4[n][k])): fp8_ref.gemm's derivation on
    the dequantised weights, with one scale multiply in place of two."""
    A, W = R8.E4M3[a8], dequant(elems, scales)
    s = np.asarray(sa, np.float64)[:, None]
    v, mag = s * (A @ W.T), np.abs(s) * (np.abs(A) @ np.abs(W).T)
    e = (2 * a8.shape[1] + 1) * R8.U32 * mag
    terms = 0
    for t in (None if bias is None else np.asarray(bias, np.float64)[None, :], None if residual is None else np.asarray(residual, np.float64)):
        if t is not None:
            v, mag, terms = v + t, mag + np.abs(t), terms + 1
    e = e + (terms + 1) * R8.U32 * mag
    if epi == R8.EPI_GEGLU:
        a, g, ea, eg = v[:, 0::2], v[:, 1::2], e[:, 0::2], e[:, 1::2]
        gl = R8.gelu_tanh64(g)
        arg = np.abs(np.sqrt(2.0 / np.pi) * 2.0 * np.log2(np.e) * (g + 0.044715 * g ** 3))
        v = a * gl
        e = np.abs(gl) * ea + (np.abs(a) + ea) * R8.GELU_DMAX * eg + np.abs(v) * (6.0 + 4.0 * arg) * R8.U32
    return v, 2.0 ** -11 * np.abs(v) + (1.0 + 2.0 ** -11) * e + 2.0 ** -25
