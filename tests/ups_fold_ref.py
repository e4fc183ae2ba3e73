"""The upsample fold stated in numpy (tests/test_ups_fold_cpu.py, tests/test_gpu_ups_fold.py).

A 3x3 convolution (pad 1) of a nearest-2x upsampled image reads, for output pixel (2 yi + py, 2 xi + px), source rows {yi - 1, yi}
through kernel rows {0}, {1, 2} when py = 0 and rows {yi, yi + 1} through {0, 1}, {2} when py = 1; columns alike.  So it is four 2x2
convolutions of the source, one per parity q = 2 py + px, whose weights are sums of up to four of the 3x3 ones.  Sums are made in
float64 (exact for fp16 terms) and cast to float16 ONCE."""
import numpy as np

GROUPS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}   # parity -> kernel rows (columns) summed into 2x2 tap 0 / 1


def fold64(w):
    """w [O][3][3][I] (any float dtype) -> float64 [4][O][2][2][I], unrounded"""
    w = np.asarray(w).astype(np.float64)
    out = np.empty((4, w.shape[0], 2, 2, w.shape[3]), np.float64)
    with np.errstate(invalid="ignore"):
        for q in range(4):
            for k2h in range(2):
                for k2w in range(2):
                    terms = [w[:, kh, kw, :] for kh in GROUPS[q >> 1][k2h] for kw in GROUPS[q & 1][k2w]]
                    s = terms[0].copy()   # the first term as it is: a lone -0 stays -0
                    for t in terms[1:]:
                        s = s + t
                    out[q, :, k2h, k2w, :] = s
    return out


def fold16(w16):
    """fp16 [O][3][3][I] -> fp16 [4][O][2][2][I]: the float64 sums rounded once, nearest-even"""
    with np.errstate(over="ignore", invalid="ignore"):
        return fold64(w16).astype(np.float16)


def tile_major(f16):
    """[4][O][2][2][I] -> the device layout: per parity the [O][4 I] matrix K-tile-major, [4][4 I / 64][O][64]"""
    q, O = f16.shape[:2]
    K = f16.shape[2] * f16.shape[3] * f16.shape[4]
    return np.ascontiguousarray(f16.reshape(q, O, K // 64, 64).transpose(0, 2, 1, 3))


def gather2x2(x, q):
    """x [B][Hs][Ws][C] float64 -> [B][Hs][Ws][4 C]: for every source position (yi, xi) the 2x2 source pixels that output pixel
    (2 yi + py, 2 xi + px) of parity q reads, zero outside the image, taps in (kh2, kw2) order"""
    B, Hs, Ws, Cn = x.shape
    py, px = q >> 1, q & 1
    p = np.zeros((B, Hs + 2, Ws + 2, Cn), x.dtype)
    p[:, 1:-1, 1:-1] = x
    taps = [p[:, py + kh:py + kh + Hs, px + kw:px + kw + Ws] for kh in range(2) for kw in range(2)]  # padded row yi + py + kh = source row yi - 1 + py + kh
    return np.concatenate(taps, axis=-1)
