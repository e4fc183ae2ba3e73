"""Token merging restated in numpy: the hash and the 2 x 2 partition of include/tsd.h in integers, the float64 cosine matrix with the error
bound the device's fp32 arithmetic must meet, the plan (selection and tables) from node_max BITS, and the merge / unmerge in float64."""
import numpy as np

U32 = 0xFFFFFFFF
EPS32, EPS16 = 2.0 ** -24, 2.0 ** -11        # unit roundoffs


def tome_hash(seed, cell):
    x = (seed ^ (cell * 0x9E3779B9)) & U32
    x = ((x ^ (x >> 16)) * 0x85EBCA6B) & U32
    x = ((x ^ (x >> 13)) * 0xC2B2AE35) & U32
    return x ^ (x >> 16)


def partition(H, W, seed):
    dst, src = [], []   # dst tokens [Nd] in cell order, src tokens [Ns]: source 3 c + k is the k-th other token of cell c in raster order
    for c in range((H // 2) * (W // 2)):
        cy, cx = divmod(c, W // 2)
        p = tome_hash(seed, c) & 3 if seed else 0
        cell = [(2 * cy + (q >> 1)) * W + 2 * cx + (q & 1) for q in range(4)]
        dst.append(cell[p])
        src += [t for q, t in enumerate(cell) if q != p]
    return np.array(dst), np.array(src)


def merged_count(ratio, N):
    return 8 * int(np.floor(float(np.float32(ratio)) * N / 8.0))


def cosine(x, dst, src):
    x = x.astype(np.float64)   # -> float64 score matrix [Ns][Nd] of one sample's fp16 rows; a zero row has inverse norm 0
    n = np.sqrt((x * x).sum(1))
    inv = np.divide(1.0, n, out=np.zeros_like(n), where=n > 0)
    return (x[src] @ x[dst].T) * inv[src, None] * inv[dst][None]


def score_bound(C):
    """|device score - float64 score| <= this.  The dot product is a sum of C exact fp16 x fp16 products accumulated in fp32 in some
    order: |error| <= gamma_C sum|a_k b_k| <= gamma_C |a||b| (Cauchy-Schwarz), gamma_C = C u / (1 - C u).  Each squared norm likewise
    carries a relative gamma_C, halved by the square root, plus one rounding each for sqrt and the reciprocal: (C / 2 + 2) u per inverse
    norm.  Two multiplications by the inverse norms add 2 u.  |score| <= 1, so in sum (C + 2 (C / 2 + 2) + 2) u, taken with a factor
    (1 + 1e-3) for the second-order terms."""
    return (2 * C + 6) * EPS32 * (1 + 1e-3)


def score_typical(C):
    """The same terms as score_bound under random-sign rounding errors: sqrt(C) in place of C.  Reported beside the bound, not asserted."""
    return (2 * np.sqrt(C) + 6) * EPS32


def model_inputs(LH, LW, B=2, kind="diffusion_sd15_torch"):
    """The model tests' shared draw at half weight on a +-1.5 checkerboard of 8 x 8 blocks; odd samples negated."""
    import freeu_ref as F
    lat, ctx, temb = F.model_inputs(kind, LH, LW)
    blocks = np.kron(np.where(np.add.outer(np.arange(-(-LH // 8)), np.arange(-(-LW // 8))) % 2 == 0, 1.5, -1.5), np.ones((8, 8)))[:LH, :LW]
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)[:, None, None, None]
    return ((0.5 * lat + blocks) * sign).astype(np.float32), np.repeat(ctx, B, 0), np.repeat(temb, B, 0)


def plan(node_max, node_idx, H, W, r, seed):
    """One sample: node_max float32 [Ns] (the DEVICE's bits), node_idx [Ns] -> (row_of [N], start [N - r + 1], members [N]).  Integer
    arithmetic: the r largest values, on equal values the smaller source index first (-0 counts as +0)."""
    dst, src = partition(H, W, seed)
    N, Nd, Ns = H * W, len(dst), len(src)
    v = node_max.astype(np.float32) + np.float32(0)            # -0 -> +0
    order = np.lexsort((np.arange(Ns), -v.astype(np.float64)))
    merged = np.zeros(Ns, bool)
    merged[order[:r]] = True
    keep = Ns - r
    row_of = np.empty(N, np.int64)
    row_of[src[~merged]] = np.arange(keep)
    row_of[dst] = keep + np.arange(Nd)
    row_of[src[merged]] = keep + node_idx[merged]
    rows = [[] for _ in range(N - r)]
    for t in range(N):
        rows[row_of[t]].append(t)
    start = np.concatenate([[0], np.cumsum([len(m) for m in rows])])
    return row_of, start, np.concatenate(rows)


def merge(x, start, members):
    """One sample: (float64 member means [rows][C], member counts, element-wise bound of the device's rows: count - 1 fp32 additions and
    one division - count u sum|x| / count - plus half an fp16 ulp of the result, u16 (mean|x| + that) and half the smallest subnormal)."""
    x, cnt = x.astype(np.float64), np.diff(start)
    mean, s = (np.add.reduceat(v[members], start[:-1], axis=0) / cnt[:, None] for v in (x, np.abs(x)))
    e32 = cnt[:, None] * EPS32 * s * (1 + 1e-3)
    return mean, cnt, e32 + EPS16 * (s + e32) + 2.0 ** -25
