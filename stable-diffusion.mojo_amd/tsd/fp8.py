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


@contextlib.contextmanager
def ff_fp8_scope(diffusion, ff_fp8):
    """`generate(ff_fp8=...)`: None leaves the model as it is; True / False sets the switch, and the previous setting is back on every way out."""
    if ff_fp8 is None:
        yield
        return
    prev = diffusion.ff_fp8
    diffusion.set_ff_fp8(ff_fp8)
    try:
        yield
    finally:
        diffusion.set_ff_fp8(prev)
