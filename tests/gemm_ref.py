"""fp64 reference and element-wise error bound for one GEMM / conv3x3 launch of csrc/kernels_gemm.hip (test infrastructure).

A launch is a descriptor: the int64 TSD_GD_* fields of include/tsd.h, one per GemmArgs field, parsed from the header so the two
sides cannot drift.  Operands are flat numpy arrays in the device layout (pitches, batch strides) - fp16 for A0 / A1 / A2 / W /
Wt1 / R, fp32 for the bias and the row vector - exactly what tsd_debug_gemm_run uploads; W is row-major [N][KW] (KW = 9*Cin for a
convolution, K for a dense GEMM) whatever the launch reads.  Elements that no launch may read (pitch gaps) hold NaN, so an
over-read shows up as a non-finite output.

`reference(desc, ops, rows)` computes, in float64 from those fp16 values, what the kernel computes for the selected output rows:

    v = out_scale * sum_k a[m][k] w[n][k] + bias[m] + bias[n] + rowvec[(m / rows_per_batch) * rowvec_ld + n] + R[m'][n]

(m' = m, or the pixel of the 2x-upsampled (Ho/2, Wo/2) residual under EPI_RES_UPS), then either GEGLU on the interleaved
(a, g) column pairs, out[m][n/2] = a * gelu_tanh(g), or the plain store; with a V^T tail the columns n >= vt_n0 go to
Vt[(m / vt_S) * vt_sB + (n - vt_n0) * vt_ld + m % vt_S] instead of C.

The bound (`bound`) follows the rounding points of the kernel, u = 2^-24 (fp32 unit roundoff):
  * products of two fp16 values are exact in fp32; the K-long fp32 accumulation (MFMA adds, the split-K hand-off) loses at
    most K * u' per add relative to the sum of |products|, and u' = 2u because the matrix core's internal adds may truncate
    instead of rounding: e_acc = 2 K u |out_scale| sum_k |a||w|.  (The scale multiply adds one more u |out_scale * acc|.)
  * every epilogue add (bias_m, bias_n, rowvec, residual) rounds once in fp32: at most u times the running magnitude, bounded
    by S = |out_scale| sum|a||w| + |bias_m| + |bias_n| + |rowvec| + |r|, so e_add = (terms + 1) u S.
  * e32 = e_acc + e_add is the error of the fp32 value y32 the kernel stores or rounds.  The fp16 store adds at most
    2^-11 |y32| <= 2^-11 (|ref| + e32) (round to nearest), plus 2^-25 in fp16's subnormal range.  EPI_OUT_F32 drops that term.
  * GEGLU: with e_a, e_g the fp32 errors of the two columns, |a gelu(g) - a' gelu(g')| <= |gelu(g)| e_a + (|a| + e_a) max|gelu'| e_g
    (max |gelu_tanh'| < 1.13), plus gelu_tanh_f's own error: its exp2 / rcp are 1-ulp approximations and the argument
    c (x + 0.044715 x^3) carries a few roundings, which move exp2's result by ln2 |arg| ulps - (6 + 4 |arg|) u relative to the
    product covers them and the final multiply.
So the bound is |y - ref| <= 2^-11 |ref| + (1 + 2^-11) e + 2^-25 with e the fp32 error above.  With operands scaled so that the
product, bias, row vector and residual are of the same order, a missing, doubled or misplaced epilogue term is far above it.

GroupNorm statistics (EPI_GNSTATS) are checked against fp64 sums over the device's own fp16 output (what the kernel sums):
per (sample, 32-row slab, group) sum x and sum x^2, each an fp32 sum of 32 * cpg terms.
"""
import os
import re

import numpy as np

import replay
from replay import NAN16, NAN32, bits_f32, f32_bits

_COMMON = os.path.join(replay.ROOT, "stable-diffusion.mojo_amd", "csrc", "common.h")
U32 = 2.0 ** -24
GELU_DMAX = 1.13


def _parse():
    txt = replay.header()
    gd, go = replay.enums(txt, {"TSD_GD_": "tsd_gemm_desc_field", "TSD_GO_": "tsd_gemm_operand"})
    ctxt = re.sub(r"//[^\n]*", "", open(_COMMON).read())
    epi = {k: int(v) for k, v in re.findall(r"\bEPI_([A-Z0-9_]+)\s*=\s*(\d+)", ctxt)}
    return gd, go, replay.version(txt, "TSD_GD_VERSION_1"), epi


GD, GO, GD_VERSION, EPI = _parse()
COUNT = GD["COUNT"]
GP, = replay.enums(replay.header(), {"TSD_GP_": "tsd_gemm_plan_field"})  # fields of tsd_debug_gemm_plan
# tile configurations (csrc/gemm_tiles.h) by column family: 160-wide tiles, 128-wide tiles, the thin N <= 16 ones
N160 = (0, 1, 5, 6, 7, 11, 45, 46, 47, 51, 54)
N128 = (2, 3, 8, 9, 10, 13, 48, 49, 50, 53, 55)
THIN = (4, 24)
INPUTS = ("A0", "A1", "A2", "W", "WT1", "R", "BIAS", "ROWVEC")
OUTPUTS = ("C", "VT", "GN")


def new_desc(**f):
    """Descriptor with defaults (batch 1, out_scale 1, one row per batch, pad 1, stride 1); keys are TSD_GD_* names, lower case."""
    d = np.zeros(COUNT, np.int64)
    d[GD["VERSION"]] = GD_VERSION
    d[GD["BATCH"]] = 1
    d[GD["OUT_SCALE"]] = f32_bits(1.0)
    d[GD["ROWS_PER_BATCH"]] = 1
    d[GD["STRIDE"]] = 1
    d[GD["PAD"]] = 1
    d[GD["CFG"]] = -1
    for k, v in f.items():
        if k == "out_scale":
            v = f32_bits(v)
        d[GD[k.upper()]] = int(v)
    return d


def conv_desc(B, Hs, Ws, Cin, N, stride=1, pad=1, pad_br=None, ups=0, Cin1=0, Cin2=0, lda0=None, lda1=None, lda2=None,
              ldc=None, ldr=None, **f):
    """conv3x3 over B images [Hs][Ws][lda0] with top/left padding `pad` and bottom/right `pad_br` (default = pad)."""
    pad_br = pad if pad_br is None else pad_br
    Hi, Wi = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
    Ho, Wo = (Hi + pad + pad_br - 3) // stride + 1, (Wi + pad + pad_br - 3) // stride + 1
    K = 9 * Cin + Cin1 + Cin2
    return new_desc(conv=1, m=B * Ho * Wo, n=N, k=K, k0=K, hs=Hs, ws=Ws, ho=Ho, wo=Wo, cin=Cin, stride=stride, pad=pad, ups=ups,
                    cin1=Cin1, cin2=Cin2, lda0=lda0 or Cin, lda1=(lda1 or Cin1) if Cin1 else 0, lda2=(lda2 or Cin2) if Cin2 else 0,
                    ldw=9 * Cin, ldw1=Cin1 + Cin2, ldc=ldc or N, ldr=ldr or N, **f)


def dense_desc(M, N, K, K0=None, lda0=None, lda1=None, ldw=None, ldc=None, ldr=None, **f):
    K0 = K if K0 is None else K0
    geglu = f.get("epi", 0) & EPI["GEGLU"]
    return new_desc(conv=0, m=M, n=N, k=K, k0=K0, lda0=lda0 or K0, lda1=(lda1 or K - K0) if K0 < K else 0, ldw=ldw or K,
                    ldc=ldc or (N // 2 if geglu else N), ldr=ldr or N, **f)


def _g(d, k):
    return int(d[GD[k]])


def out_scale(d):
    return bits_f32(_g(d, "OUT_SCALE"))


def c_cols(d):
    if _g(d, "VT"):
        return _g(d, "VT_N0")
    return _g(d, "N") // 2 if _g(d, "EPI") & EPI["GEGLU"] else _g(d, "N")


def kw(d):
    return 9 * _g(d, "CIN") if _g(d, "CONV") else _g(d, "K")


def samples(d):
    return _g(d, "M") // (_g(d, "HO") * _g(d, "WO")) if _g(d, "CONV") else 1


def dtype_of(s, d):
    """numpy type of operand slot s (the entry's gd_elem_bytes)."""
    f32 = s in ("BIAS", "ROWVEC", "GN") or (s == "C" and _g(d, "EPI") & EPI["OUT_F32"])
    return np.float32 if f32 else np.float16


def extents(d):
    """Element extent of every operand slot (0 = unused): the restatement of the entry's sizing, held against it on the GPU."""
    e = dict.fromkeys(INPUTS + OUTPUTS, 0)
    M, N, K, K0, B, epi = (_g(d, k) for k in ("M", "N", "K", "K0", "BATCH", "EPI"))
    sA, sW, sC, sR = (_g(d, k) for k in ("SA", "SW", "SC", "SR"))
    if _g(d, "CONV"):
        px = samples(d) * _g(d, "HS") * _g(d, "WS")
        e["A0"] = (px - 1) * _g(d, "LDA0") + _g(d, "CIN")
        c1, c2 = _g(d, "CIN1"), _g(d, "CIN2")
        if c1:
            e["A1"] = (px - 1) * _g(d, "LDA1") + c1
            if c2:
                e["A2"] = (px - 1) * _g(d, "LDA2") + c2
            e["WT1"] = (N - 1) * _g(d, "LDW1") + c1 + c2
    else:
        e["A0"] = (B - 1) * sA + (M - 1) * _g(d, "LDA0") + K0
        if K0 < K:
            e["A1"] = (B - 1) * sA + (M - 1) * _g(d, "LDA1") + K - K0
    e["W"] = N * kw(d) if _g(d, "W_KTS") else (B - 1) * sW + (N - 1) * _g(d, "LDW") + kw(d)
    e["C"] = (B - 1) * sC + (M - 1) * _g(d, "LDC") + c_cols(d)
    if epi & (EPI["BIAS_N"] | EPI["BIAS_M"]):
        e["BIAS"] = max(N if epi & EPI["BIAS_N"] else 0, M if epi & EPI["BIAS_M"] else 0)
    if epi & EPI["ROWVEC"]:
        e["ROWVEC"] = ((M - 1) // _g(d, "ROWS_PER_BATCH")) * _g(d, "ROWVEC_LD") + N
    if epi & EPI["RESIDUAL"]:
        if _g(d, "ALIAS") & 1:
            e["R"] = e["C"]
        else:
            rows = M
            if _g(d, "CONV") and epi & EPI["RES_UPS"]:
                rows = samples(d) * (_g(d, "HO") // 2) * (_g(d, "WO") // 2)
            e["R"] = (B - 1) * sR + (rows - 1) * _g(d, "LDR") + N
    if _g(d, "VT"):
        S = _g(d, "VT_S")
        e["VT"] = (M // S - 1) * _g(d, "VT_SB") + (N - _g(d, "VT_N0") - 1) * _g(d, "VT_LD") + S
    if epi & EPI["GNSTATS"]:
        e["GN"] = (M // _g(d, "GN_RPS")) * _g(d, "GN_NSLAB") * _g(d, "GN_GROUPS") * 2
    return e


def _mask_rows(ext, starts, width):
    m = np.zeros(ext, bool)
    starts = np.asarray(starts, np.int64)
    if len(starts) == 1 or (np.diff(starts) == width).all():  # packed rows: one contiguous run
        m[starts[0]:starts[-1] + width] = True
        return m
    idx = (np.asarray(starts, np.int64)[:, None] + np.arange(width)[None, :]).ravel()
    m[idx] = True
    return m


def input_masks(d):
    """Elements of each input the launch may read (True); the rest are pitch gaps."""
    e = extents(d)
    M, N, K, K0, B = (_g(d, k) for k in ("M", "N", "K", "K0", "BATCH"))
    out = {}
    rows_b = lambda s, ld, n_rows: (np.arange(B)[:, None] * s + np.arange(n_rows)[None, :] * ld).ravel()  # noqa: E731
    if _g(d, "CONV"):
        px = samples(d) * _g(d, "HS") * _g(d, "WS")
        out["A0"] = _mask_rows(e["A0"], np.arange(px) * _g(d, "LDA0"), _g(d, "CIN"))
        if e["A1"]:
            out["A1"] = _mask_rows(e["A1"], np.arange(px) * _g(d, "LDA1"), _g(d, "CIN1"))
        if e["A2"]:
            out["A2"] = _mask_rows(e["A2"], np.arange(px) * _g(d, "LDA2"), _g(d, "CIN2"))
        if e["WT1"]:
            out["WT1"] = _mask_rows(e["WT1"], np.arange(N) * _g(d, "LDW1"), _g(d, "CIN1") + _g(d, "CIN2"))
    else:
        out["A0"] = _mask_rows(e["A0"], rows_b(_g(d, "SA"), _g(d, "LDA0"), M), K0)
        if e["A1"]:
            out["A1"] = _mask_rows(e["A1"], rows_b(_g(d, "SA"), _g(d, "LDA1"), M), K - K0)
    if _g(d, "W_KTS"):
        out["W"] = np.ones(e["W"], bool)
    else:
        out["W"] = _mask_rows(e["W"], rows_b(_g(d, "SW"), _g(d, "LDW"), N), kw(d))
    for s in ("BIAS", "ROWVEC"):
        if e[s]:
            m = np.zeros(e[s], bool)
            if s == "BIAS":
                m[:] = True
            else:
                ld, rpb = _g(d, "ROWVEC_LD"), _g(d, "ROWS_PER_BATCH")
                for r in range((M - 1) // rpb + 1):
                    m[r * ld:r * ld + N] = True
            out[s] = m
    if e["R"]:
        if _g(d, "ALIAS") & 1:
            out["R"] = output_mask(d, "C")
        else:
            rows = M
            if _g(d, "CONV") and _g(d, "EPI") & EPI["RES_UPS"]:
                rows = samples(d) * (_g(d, "HO") // 2) * (_g(d, "WO") // 2)
            out["R"] = _mask_rows(e["R"], rows_b(_g(d, "SR"), _g(d, "LDR"), rows), N)
    return out


def output_mask(d, slot):
    e = extents(d)[slot]
    M, N, B = _g(d, "M"), _g(d, "N"), _g(d, "BATCH")
    if slot == "C":
        starts = (np.arange(B)[:, None] * _g(d, "SC") + np.arange(M)[None, :] * _g(d, "LDC")).ravel()
        return _mask_rows(e, starts, c_cols(d))
    if slot == "VT":
        S, n0 = _g(d, "VT_S"), _g(d, "VT_N0")
        starts = (np.arange(M // S)[:, None] * _g(d, "VT_SB") + np.arange(N - n0)[None, :] * _g(d, "VT_LD")).ravel()
        return _mask_rows(e, starts, S)
    return np.ones(e, bool)


def make_operands(d, seed, scale=None):
    """Seeded operands in the device layout, NaN in every pitch gap.  Default scales put the product (A, W ~ U(-1, 1) / sqrt(K)
    per term), the biases, the row vector and the residual at the same order (~0.3 - 0.6)."""
    rng = np.random.default_rng(seed)
    K = _g(d, "K")
    sc = {"A0": 1.0, "A1": 1.0, "A2": 1.0, "W": 1.7 / np.sqrt(K), "WT1": 1.7 / np.sqrt(K), "R": 0.5, "BIAS": 0.5, "ROWVEC": 0.5}
    if scale:
        sc.update(scale)
    masks = input_masks(d)
    ops = {}
    for s, n in extents(d).items():
        if not n or s in OUTPUTS:
            continue
        dt = dtype_of(s, d)
        x = (rng.uniform(-1.0, 1.0, n) * sc[s]).astype(dt)
        x[~masks[s]] = NAN32 if dt == np.float32 else NAN16
        ops[s] = x
    return ops


def _rows_geometry(d, rows):
    """(batch index, row in batch) of flat output rows r in [0, batch * M)."""
    M = _g(d, "M")
    rows = np.asarray(rows, np.int64)
    return rows // M, rows % M


def gather_a(d, ops, rows):
    """A[r][k] in float64 for the selected flat rows (conv: the implicit im2col, zero outside the image)."""
    rows = np.asarray(rows, np.int64)
    bz, m = _rows_geometry(d, rows)
    K, K0 = _g(d, "K"), _g(d, "K0")
    A = np.zeros((len(rows), K), np.float64)
    if not _g(d, "CONV"):
        a0 = ops["A0"].astype(np.float64)
        base0 = bz * _g(d, "SA") + m * _g(d, "LDA0")
        A[:, :K0] = a0[base0[:, None] + np.arange(K0)[None, :]]
        if K0 < K:
            a1 = ops["A1"].astype(np.float64)
            base1 = bz * _g(d, "SA") + m * _g(d, "LDA1")
            A[:, K0:] = a1[base1[:, None] + np.arange(K - K0)[None, :]]
        return A
    Hs, Ws, Ho, Wo, Cin = (_g(d, k) for k in ("HS", "WS", "HO", "WO", "CIN"))
    st, pad, ups = _g(d, "STRIDE"), _g(d, "PAD"), _g(d, "UPS")
    b, rem = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    He, We = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
    a0 = ops["A0"].astype(np.float64)
    for t in range(9):
        kh, kwi = divmod(t, 3)
        iy, ix = oy * st - pad + kh, ox * st - pad + kwi
        ok = (iy >= 0) & (iy < He) & (ix >= 0) & (ix < We)
        sy, sx = (iy >> 1, ix >> 1) if ups else (iy, ix)
        pix = np.where(ok, (b * Hs + sy) * Ws + sx, 0)
        v = a0[pix[:, None] * _g(d, "LDA0") + np.arange(Cin)[None, :]]
        A[:, t * Cin:(t + 1) * Cin] = np.where(ok[:, None], v, 0.0)
    c1, c2 = _g(d, "CIN1"), _g(d, "CIN2")
    if c1:
        pix = (b * Hs + oy) * Ws + ox
        A[:, 9 * Cin:9 * Cin + c1] = ops["A1"].astype(np.float64)[pix[:, None] * _g(d, "LDA1") + np.arange(c1)[None, :]]
        if c2:
            A[:, 9 * Cin + c1:] = ops["A2"].astype(np.float64)[pix[:, None] * _g(d, "LDA2") + np.arange(c2)[None, :]]
    return A


def weight(d, ops, bz=0):
    """W[n][k] in float64 ([N][K]: the nine taps, then the fused skip's Cin1 + Cin2 channels)."""
    N, KW = _g(d, "N"), kw(d)
    w = ops["W"].astype(np.float64)
    if _g(d, "W_KTS"):
        Wm = w.reshape(N, KW)
    else:
        Wm = w[bz * _g(d, "SW") + np.arange(N)[:, None] * _g(d, "LDW") + np.arange(KW)[None, :]]
    c = _g(d, "CIN1") + _g(d, "CIN2") if _g(d, "CONV") else 0
    if c:
        w1 = ops["WT1"].astype(np.float64)[np.arange(N)[:, None] * _g(d, "LDW1") + np.arange(c)[None, :]]
        Wm = np.concatenate([Wm, w1], axis=1)
    return Wm


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def reference(d, ops, rows):
    """Returns (v, e32, cout): v [len(rows)][N] fp64 pre-store values (after GEGLU: [len(rows)][N/2]), e32 their fp32 error
    bound, cout the column count of the result."""
    rows = np.asarray(rows, np.int64)
    bz, m = _rows_geometry(d, rows)
    N, K, epi = _g(d, "N"), _g(d, "K"), _g(d, "EPI")
    s = out_scale(d)
    A = gather_a(d, ops, rows)
    acc = np.empty((len(rows), N))
    sabs = np.empty((len(rows), N))
    for b in np.unique(bz):
        sel = bz == b
        Wm = weight(d, ops, int(b))
        acc[sel] = A[sel] @ Wm.T
        sabs[sel] = np.abs(A[sel]) @ np.abs(Wm).T
    v = s * acc
    mag = abs(s) * sabs
    e = 2 * K * U32 * mag + U32 * mag
    terms = 0
    if epi & EPI["BIAS_M"]:
        t = ops["BIAS"].astype(np.float64)[m][:, None]
        v, mag, terms = v + t, mag + np.abs(t), terms + 1
    if epi & EPI["BIAS_N"]:
        t = ops["BIAS"].astype(np.float64)[:N][None, :]
        v, mag, terms = v + t, mag + np.abs(t), terms + 1
    if epi & EPI["ROWVEC"] and _g(d, "CONV"):
        rv = ops["ROWVEC"].astype(np.float64)
        t = rv[(m // _g(d, "ROWS_PER_BATCH"))[:, None] * _g(d, "ROWVEC_LD") + np.arange(N)[None, :]]
        v, mag, terms = v + t, mag + np.abs(t), terms + 1
    if epi & EPI["RESIDUAL"]:
        rrow = m
        if _g(d, "CONV") and epi & EPI["RES_UPS"]:
            Ho, Wo = _g(d, "HO"), _g(d, "WO")
            bb, rem = m // (Ho * Wo), m % (Ho * Wo)
            oy, ox = rem // Wo, rem % Wo
            rrow = (bb * (Ho // 2) + oy // 2) * (Wo // 2) + ox // 2
        R = ops["R"].astype(np.float64)
        t = R[(bz * _g(d, "SR") + rrow * _g(d, "LDR"))[:, None] + np.arange(N)[None, :]]
        v, mag, terms = v + t, mag + np.abs(t), terms + 1
    e = e + (terms + 1) * U32 * mag
    if epi & EPI["GEGLU"] and not _g(d, "CONV"):
        a, g = v[:, 0::2], v[:, 1::2]
        ea, eg = e[:, 0::2], e[:, 1::2]
        gl = gelu_tanh64(g)
        arg = np.abs(np.sqrt(2.0 / np.pi) * 2.0 * np.log2(np.e) * (g + 0.044715 * g ** 3))
        y = a * gl
        ey = np.abs(gl) * ea + (np.abs(a) + ea) * GELU_DMAX * eg + np.abs(y) * (6.0 + 4.0 * arg) * U32
        return y, ey, N // 2
    return v, e, N


def bound(d, ref, e32):
    if _g(d, "EPI") & EPI["OUT_F32"]:
        return e32 + 2.0 ** -140
    return 2.0 ** -11 * np.abs(ref) + (1.0 + 2.0 ** -11) * e32 + 2.0 ** -25


def device_rows(d, out, rows, slot="C"):
    """The device's values at the selected rows: C [len(rows)][cols] or the Vt tail [len(rows)][N - vt_n0], as float64."""
    rows = np.asarray(rows, np.int64)
    bz, m = _rows_geometry(d, rows)
    if slot == "VT":
        S, n0, N = _g(d, "VT_S"), _g(d, "VT_N0"), _g(d, "N")
        idx = ((m // S) * _g(d, "VT_SB") + m % S)[:, None] + np.arange(N - n0)[None, :] * _g(d, "VT_LD")
        return out.astype(np.float64)[idx]
    cols = c_cols(d)
    return out.astype(np.float64)[(bz * _g(d, "SC") + m * _g(d, "LDC"))[:, None] + np.arange(cols)[None, :]]


def check(d, ops, outs, rows):
    """Every sampled element of C (and Vt) within the bound.  Returns a list of failure strings (empty: pass)."""
    rows = np.asarray(sorted(set(int(r) for r in rows)), np.int64)
    ref, e32, _ = reference(d, ops, rows)
    bd = bound(d, ref, e32)
    fails = []
    parts = [("C", ref[:, :c_cols(d)], bd[:, :c_cols(d)])]
    if _g(d, "VT"):
        n0 = _g(d, "VT_N0")
        parts.append(("VT", ref[:, n0:], bd[:, n0:]))
    for slot, r, b in parts:
        got = device_rows(d, outs[slot], rows, slot)
        err = np.abs(got - r)
        bad = ~(err <= b)  # NaN fails
        if bad.any():
            i, j = np.argwhere(bad)[0]
            fails.append(f"{slot}: {int(bad.sum())} of {bad.size} elements outside the bound; first row {rows[i]} col {j}: "
                         f"got {got[i, j]!r} ref {r[i, j]:.6g} bound {b[i, j]:.3g}")
    return fails


def gn_reference(d, c_out):
    """fp64 (sum, sum of squares) per (sample, 32-row slab, group) of the device's fp16 C, laid out like gn_part."""
    M, N, G, rps, ns = (_g(d, k) for k in ("M", "N", "GN_GROUPS", "GN_RPS", "GN_NSLAB"))
    cpg = N // G
    y = device_rows(d, c_out, np.arange(M))  # [M][N]
    y = y.reshape(M // rps, rps // 32, 32, G, cpg)[:, :ns]
    s1 = y.sum(axis=(2, 4))
    s2 = (y * y).sum(axis=(2, 4))
    return np.stack([s1, s2], axis=-1).ravel(), np.stack([np.abs(y).sum(axis=(2, 4)), s2], axis=-1).ravel(), 32 * cpg


def check_gn(d, c_out, gn):
    """The partial sums: fp32 sums of 32 * cpg fp16-exact terms (squares rounded once) - n u per term magnitude, u' = 2u."""
    ref, mag, n = gn_reference(d, c_out)
    b = 2.0 * (n + 1) * U32 * mag + 2.0 ** -60
    err = np.abs(gn.astype(np.float64) - ref)
    bad = ~(err <= b)
    if bad.any():
        i = int(np.argmax(bad))
        return [f"GN: {int(bad.sum())} of {bad.size} partials off; first index {i}: got {gn[i]!r} ref {ref[i]:.6g} bound {b[i]:.3g}"]
    return []


def sample_rows(d, seed, n_random=256):
    """Row sample: first and last row of every 64-row block, sample boundaries +- 1, image-border pixels of conv outputs,
    and `n_random` seeded rows (flat over the batch)."""
    M, B = _g(d, "M"), _g(d, "BATCH")
    tot = M * B
    r = set()
    for s in range(0, tot, 64):
        r.update((s, min(s + 63, tot - 1)))
    if _g(d, "CONV"):
        Ho, Wo = _g(d, "HO"), _g(d, "WO")
        hw = Ho * Wo
        for b in range(M // hw):
            for x in range(Wo):
                r.update((b * hw + x, b * hw + (Ho - 1) * Wo + x))
            for y in range(Ho):
                r.update((b * hw + y * Wo, b * hw + y * Wo + Wo - 1))
        bound_step = hw
    else:
        bound_step = _g(d, "RPS_HINT") or _g(d, "GN_RPS") or _g(d, "VT_S") or M
    for s in range(0, tot + 1, max(bound_step, 1)):
        r.update(x for x in (s - 1, s, s + 1) if 0 <= x < tot)
    for s in range(0, tot + 1, M):
        r.update(x for x in (s - 1, s, s + 1) if 0 <= x < tot)
    rng = np.random.default_rng(seed)
    r.update(int(x) for x in rng.integers(0, tot, n_random))
    return np.array(sorted(r), np.int64)


# ---- the launch tables of tests/test_gpu_gemm_ref.py (shared with tests/jitter_manifest.py: the same cases under perturbed timing) ----
PROD_CONV = EPI["BIAS_N"] | EPI["RESIDUAL"]


def _sweep_cases():
    """(name, descriptor, configurations that take it)."""
    out = []

    def both(name, make):  # one shape per column family: N = 320 (160-wide tiles) and N = 256 / 132 (128-wide)
        out.append((name + "/n160", make(320), N160 + N128))
        out.append((name + "/n128", make(256), N128))

    # M: conv images that straddle tiles (12 x 12 per sample, B = 3), stride 2 on odd / even sizes (Wo 13), H != W, tiny images
    both("conv_b3_12x12_res_rowvec", lambda N: conv_desc(B=3, Hs=12, Ws=12, Cin=64, N=N, epi=PROD_CONV | EPI["ROWVEC"],
                                                           rowvec_ld=N, rows_per_batch=144))
    both("conv_s2_odd_wo13", lambda N: conv_desc(B=1, Hs=25, Ws=25, Cin=64, N=N, stride=2, epi=EPI["BIAS_N"]))
    both("conv_s2_even_pad01", lambda N: conv_desc(B=2, Hs=16, Ws=10, Cin=128, N=N, stride=2, pad=0, pad_br=1, epi=EPI["BIAS_N"]))
    both("conv_pad0_hw", lambda N: conv_desc(B=1, Hs=7, Ws=11, Cin=64, N=N, pad=0, epi=EPI["BIAS_N"] | EPI["OUT_F32"], out_scale=0.5))
    both("conv_ups_wo24_resups", lambda N: conv_desc(B=2, Hs=12, Ws=12, Cin=64, N=N, ups=1, epi=PROD_CONV | EPI["RES_UPS"]))
    both("conv_1x1_2x2", lambda N: conv_desc(B=4, Hs=2, Ws=2, Cin=64, N=N, epi=EPI["BIAS_N"], ldc=N + 8))
    both("conv_cin320_wkts", lambda N: conv_desc(B=1, Hs=8, Ws=8, Cin=320, N=N, epi=PROD_CONV, w_kts=1))
    both("conv_skip_wkts", lambda N: conv_desc(B=2, Hs=8, Ws=5, Cin=64, N=N, Cin1=128, Cin2=64, lda1=136, epi=PROD_CONV,
                                                 w_kts=1, rows_per_batch=40))
    both("conv_wo40", lambda N: conv_desc(B=1, Hs=40, Ws=40, Cin=64, N=N, epi=EPI["BIAS_N"]))
    # each epilogue flag on its own, a scaled fp16 store, the fused skip on row-major weights (its bias in the pitch-0 row vector)
    both("conv_plain", lambda N: conv_desc(B=2, Hs=6, Ws=7, Cin=64, N=N))
    both("conv_rowvec_only", lambda N: conv_desc(B=2, Hs=6, Ws=7, Cin=64, N=N, epi=EPI["ROWVEC"], rowvec_ld=N, rows_per_batch=42))
    both("conv_res_only_scaled", lambda N: conv_desc(B=2, Hs=6, Ws=7, Cin=64, N=N, epi=EPI["RESIDUAL"], out_scale=0.25))
    both("conv_skip_rowmajor", lambda N: conv_desc(B=2, Hs=7, Ws=6, Cin=128, N=N, Cin1=64, epi=PROD_CONV | EPI["ROWVEC"],
                                                     rowvec_ld=0, rows_per_batch=42))
    both("dense_biasm_only", lambda N: dense_desc(M=70, N=N, K=128, epi=EPI["BIAS_M"]))
    both("dense_geglu_only", lambda N: dense_desc(M=70, N=N, K=128, epi=EPI["GEGLU"]))
    both("dense_f32_only", lambda N: dense_desc(M=70, N=N, K=128, epi=EPI["OUT_F32"]))
    both("dense_scaled_f16", lambda N: dense_desc(M=70, N=N, K=192, epi=EPI["BIAS_N"] | EPI["RESIDUAL"], out_scale=2.0))
    # dense: M below one tile and BM * t +- 1, K = 64, few K tiles, K0 at 64 and mid-K, batched strides, GEGLU, BIAS_M, f32
    both("dense_m40_k64", lambda N: dense_desc(M=40, N=N, K=64, epi=EPI["BIAS_N"]))
    both("dense_m255_k128_res_inplace", lambda N: dense_desc(M=255, N=N, K=128, epi=EPI["BIAS_N"] | EPI["RESIDUAL"], alias=1))
    both("dense_m257_concat64", lambda N: dense_desc(M=257, N=N, K=320, K0=64, lda0=72, epi=EPI["BIAS_N"] | EPI["RESIDUAL"]))
    both("dense_m129_concat_mid_wkts", lambda N: dense_desc(M=129, N=N, K=640, K0=320, epi=EPI["BIAS_N"], w_kts=1))
    both("dense_geglu", lambda N: dense_desc(M=200, N=N, K=192, epi=EPI["BIAS_N"] | EPI["GEGLU"]))
    both("dense_biasm_f32_scaled", lambda N: dense_desc(M=130, N=N, K=256, epi=EPI["BIAS_M"] | EPI["BIAS_N"] | EPI["OUT_F32"],
                                                          out_scale=0.125))
    both("dense_batched", lambda N: dense_desc(M=65, N=N, K=128, batch=3, sa=65 * 128 + 64, sw=N * 128 + 64,
                                                 sc=65 * N + 8, sr=65 * N + 16, epi=EPI["BIAS_N"] | EPI["RESIDUAL"]))
    # N % 8 == 4: the non-coalesced epilogue; partial last column tile
    out.append(("dense_n132", dense_desc(M=100, N=132, K=128, epi=EPI["BIAS_N"] | EPI["RESIDUAL"]), N128))
    out.append(("conv_n132", conv_desc(B=1, Hs=9, Ws=9, Cin=64, N=132, epi=PROD_CONV), N128))
    # thin tiles (N <= 16)
    for N in (4, 8, 16):
        out.append((f"conv_thin_n{N}", conv_desc(B=2, Hs=9, Ws=7, Cin=128, N=N, epi=EPI["BIAS_N"] | EPI["OUT_F32"]), THIN))
    out.append(("dense_thin_n12", dense_desc(M=131, N=12, K=192, epi=EPI["BIAS_N"]), THIN))
    # GroupNorm statistics: channels per group 1, 4, 8, 10, 16, 20, 40; several samples stacked in M
    for N, groups in ((320, 320), (128, 32), (256, 32), (320, 32), (512, 32), (640, 32), (1280, 32)):
        out.append((f"conv_gn_n{N}_g{groups}", conv_desc(B=3, Hs=8, Ws=8, Cin=64, N=N, epi=EPI["BIAS_N"] | EPI["GNSTATS"],
                                                           gn_groups=groups, gn_rps=64, gn_nslab=2),
                    N160 + N128 if N % 160 == 0 else N128))
    # XCD grid remap: tile grids that select xcd_n 1, 2, 4, 8 (tiles_n x tiles_m factorisations of 8)
    for N, M in ((1280, 256), (640, 512), (320, 1024), (160, 2048)):
        out.append((f"dense_xcd_n{N}", dense_desc(M=M, N=N, K=128, epi=EPI["BIAS_N"]), (0, 5, 7, 11, 51, 54)))
    # halo-x variants (opt-in): stride 1, Wo = 64, whole 128-pixel tiles
    for N in (256, 320):
        out.append((f"conv_halo_n{N}", conv_desc(B=1, Hs=4, Ws=64, Cin=64, N=N, epi=PROD_CONV), (30, 32)))
    return out


BNW = {**{c: 80 for c in N160}, **{c: 64 for c in N128}}  # wave-tile columns (FN * 16 of csrc/gemm_tiles.h); thin tiles emit no statistics

# dispatcher-only modes: (name, descriptor, split-K slices the dispatcher must choose)
SPLITS = [
    # rows per sample <= 64: 64-row tiles, 2 / 4 / 8 slices by K
    ("dense_rps64_k1024", dense_desc(M=256, N=1280, K=1024, epi=EPI["BIAS_N"] | EPI["RESIDUAL"], rps_hint=64), 2),
    ("dense_rps64_k2048", dense_desc(M=256, N=1280, K=2048, epi=EPI["BIAS_N"], rps_hint=64), 4),
    ("dense_rps64_k8192", dense_desc(M=256, N=1280, K=8192, epi=EPI["BIAS_N"] | EPI["RESIDUAL"], rps_hint=64), 8),
    # fused skip: slices that end inside the skip segment (18 main K tiles of 32; 9 of 21)
    ("conv_skip_4way", conv_desc(B=2, Hs=8, Ws=8, Cin=128, N=1024, Cin1=512, Cin2=384, epi=PROD_CONV, rps_hint=64), 4),
    ("conv_skip_2way", conv_desc(B=2, Hs=8, Ws=8, Cin=64, N=1280, Cin1=512, Cin2=256, epi=PROD_CONV, rps_hint=64), 2),
    # 16x16 level: 128-row tiles, K >= 4096 -> 2; at most 4 tile columns -> 4; the graph's long-K setting (K >= 8192) -> 4
    ("conv_s2_wide_4way", conv_desc(B=2, Hs=32, Ws=32, Cin=640, N=640, stride=2, epi=EPI["BIAS_N"], rps_hint=256), 4),
    ("dense_rps256_k5120", dense_desc(M=512, N=1280, K=5120, epi=EPI["BIAS_N"] | EPI["RESIDUAL"], rps_hint=256), 2),
    ("dense_rps256_k10240_big4", dense_desc(M=512, N=1280, K=10240, epi=EPI["BIAS_N"], rps_hint=256, sk_big=4), 4),
]


def _vt_desc():
    S, C_ = 256, 320
    return dense_desc(M=2 * S, N=3 * C_, K=320, ldc=2 * C_, epi=EPI["BIAS_N"], vt=1, vt_n0=2 * C_, vt_ld=S, vt_s=S, vt_sb=C_ * S,
                        rps_hint=S)
