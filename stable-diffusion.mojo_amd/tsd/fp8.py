"""The opt-in FP8 feed-forward (include/tsd.h "FP8 feed-forward"): the e4m3 row quantiser and the e4m3 GEMM alone, a linear layer through
both, and the scope `generate(ff_fp8=True)` turns the model's switch on in.  No reference counterpart."""
import contextlib

import numpy as np

from ._lib import check, f32, lib, ptr
from .utils import _ctx

EPI_NONE, EPI_GEGLU = 0, 1


def quant_rows_e4m3(x, K=None, ctx=None):
    """x float16 (M, ld), columns < K quantised (K = ld by default) -> (q uint8 (M, Kp), scale float32 (M,)), Kp = K rounded up to 128:
    per row scale = max|x| / 448 and q = e4m3(x * 448 / max|x|), OCP e4m3 bytes, the pad bytes zero (`tsd_quant_rows_e4m3`)."""
    xa = np.ascontiguousarray(x, dtype=np.float16)
    if xa.ndim != 2:
        raise ValueError("quant_rows_e4m3: x must be (M, ld)")
    M, ld = xa.shape
    K = ld if K is None else int(K)
    q, s = np.empty((M, -(-K // 128) * 128), np.uint8), np.empty(M, np.float32)
    check(lib().tsd_quant_rows_e4m3(_ctx(ctx), xa.ctypes.data, M, K, ld, q.ctypes.data, ptr(s)))
    return q, s


def fp8_gemm(a8, sa, w8, sw, K=None, bias=None, residual=None, epi=EPI_NONE, out=None, ctx=None):
    """out (M, ldo) float16 = rn16(epi(sa[m] sw[n] sum_k a8[m][k] w8[n][k])) on e4m3 bytes a8 (M, Kp), w8 (N, Kp) (`tsd_fp8_gemm_f16`);
    bias float32 (N,), residual float16 (M, ldr), epi EPI_GEGLU: width N / 2.  `out` gives the pitch (and keeps what the launch leaves)."""
    a8, w8 = np.ascontiguousarray(a8, dtype=np.uint8), np.ascontiguousarray(w8, dtype=np.uint8)
    sa, sw = f32(sa), f32(sw)
    M, N = a8.shape[0], w8.shape[0]
    K = a8.shape[1] if K is None else int(K)
    if a8.shape[1] != -(-K // 128) * 128 or w8.shape[1] != a8.shape[1] or sa.shape != (M,) or sw.shape != (N,):
        raise ValueError("fp8_gemm: a8 (M, Kp), w8 (N, Kp) with Kp = K rounded up to 128, sa (M,), sw (N,)")
    b = None if bias is None else f32(bias)
    r = None if residual is None else np.ascontiguousarray(residual, dtype=np.float16)
    if (b is not None and b.shape != (N,)) or (r is not None and (r.ndim != 2 or r.shape[0] != M or r.shape[1] < N)):
        raise ValueError("fp8_gemm: bias (N,), residual (M, ldr >= N)")
    o = np.zeros((M, N // 2 if epi == EPI_GEGLU else N), np.float16) if out is None else np.ascontiguousarray(out, dtype=np.float16)
    check(lib().tsd_fp8_gemm_f16(_ctx(ctx), a8.ctypes.data, ptr(sa), w8.ctypes.data, ptr(sw), None if b is None else ptr(b),
                                 None if r is None else r.ctypes.data, 0 if r is None else r.shape[1], M, N, K, int(epi), o.ctypes.data, o.shape[1]))
    return o


def linear_fp8(x, w, bias=None, ctx=None):
    """y (M, N) float32 = x (M, K) . w (N, K)^T + bias with both operands quantised to e4m3 on the device (`tsd_linear_fp8_f32`)."""
    xa, wa = f32(x), f32(w)
    b = None if bias is None else f32(bias)
    y = np.empty((xa.shape[0], wa.shape[0]), np.float32)
    check(lib().tsd_linear_fp8_f32(_ctx(ctx), ptr(xa), xa.shape[0], xa.shape[1], ptr(wa), None if b is None else ptr(b), wa.shape[0], ptr(y)))
    return y


def quant_weights_mxfp4(w, K=None, ctx=None):
    """w float16 (N, ld), columns < K (a multiple of 32; ld by default) -> (elems uint8 (N, Kp / 2), scales uint8 (N, Kp / 32)), Kp = K
    rounded up to 128: OCP MXFP4, per block of 32 columns scale byte floor(log2 max|w|) - 2 + 127 and e2m1 elements, low nibble first
    (`tsd_quant_weights_mxfp4`).  A non-finite weight raises TsdError."""
    wa = np.ascontiguousarray(w, dtype=np.float16)
    if wa.ndim != 2:
        raise ValueError("quant_weights_mxfp4: w must be (N, ld)")
    N, ld = wa.shape
    K = ld if K is None else int(K)
    Kp = -(-K // 128) * 128
    e, s = np.empty((N, Kp // 2), np.uint8), np.empty((N, Kp // 32), np.uint8)
    check(lib().tsd_quant_weights_mxfp4(_ctx(ctx), wa.ctypes.data, N, K, ld, e.ctypes.data, s.ctypes.data))
    return e, s


def mxfp4_gemm(a8, sa, w4, scales, K=None, bias=None, residual=None, epi=EPI_NONE, out=None, ctx=None):
    """out (M, ldo) float16 = rn16(epi(sa[m] sum_k a8[m][k] X[n][k / 32] w4[n][k])) on e4m3 bytes a8 (M, Kp) and MXFP4 weights w4 (N, Kp / 2),
    scales (N, Kp / 32) as `quant_weights_mxfp4` gives them (`tsd_mxfp4_gemm_f16`); bias, residual, epi and `out` as for `fp8_gemm`."""
    a8, w4, scales, sa = (np.ascontiguousarray(a8, dtype=np.uint8), np.ascontiguousarray(w4, dtype=np.uint8),
                          np.ascontiguousarray(scales, dtype=np.uint8), f32(sa))
    M, N, Kp = a8.shape[0], w4.shape[0], a8.shape[1]
    K = Kp if K is None else int(K)
    if Kp != -(-K // 128) * 128 or w4.shape != (N, Kp // 2) or scales.shape != (N, Kp // 32) or sa.shape != (M,):
        raise ValueError("mxfp4_gemm: a8 (M, Kp), w4 (N, Kp / 2), scales (N, Kp / 32) with Kp = K rounded up to 128, sa (M,)")
    b = None if bias is None else f32(bias)
    r = None if residual is None else np.ascontiguousarray(residual, dtype=np.float16)
    if (b is not None and b.shape != (N,)) or (r is not None and (r.ndim != 2 or r.shape[0] != M or r.shape[1] < N)):
        raise ValueError("mxfp4_gemm: bias (N,), residual (M, ldr >= N)")
    o = np.zeros((M, N // 2 if epi == EPI_GEGLU else N), np.float16) if out is None else np.ascontiguousarray(out, dtype=np.float16)
    check(lib().tsd_mxfp4_gemm_f16(_ctx(ctx), a8.ctypes.data, ptr(sa), w4.ctypes.data, scales.ctypes.data, None if b is None else ptr(b),
                                   None if r is None else r.ctypes.data, 0 if r is None else r.shape[1], M, N, K, int(epi), o.ctypes.data, o.shape[1]))
    return o


def ff_fp8_mode(on):
    """`set_ff_fp8`'s argument -> the ABI's value: False / None 0, True 1 (e4m3 weights), "mxfp4" 2."""
    if isinstance(on, str):
        if on != "mxfp4":
            raise ValueError(f'ff_fp8: {on!r} (True, False or "mxfp4")')
        return 2
    return 1 if on else 0


@contextlib.contextmanager
def ff_fp8_scope(diffusion, ff_fp8):
    """`generate(ff_fp8=...)`: None leaves the model as it is; True / False / "mxfp4" sets the switch, and the previous setting is back on
    every way out."""
    if ff_fp8 is None:
        yield
        return
    prev = diffusion.ff_fp8
    diffusion.set_ff_fp8(ff_fp8)
    try:
        yield
    finally:
        diffusion.set_ff_fp8(prev)
