"""fp64 reference, element-wise error bound and numpy emulation for the attention core (csrc/kernels_attn.hip flash_attn_kernel<40,1>,
<40,2>, <80,1>, <160,1>; csrc/kernels_attn8.hip flash_attn8_kernel<40>) and the row-softmax kernels of csrc/kernels_elementwise.hip
(test infrastructure).

A launch is a descriptor: the int64 TSD_AD_* fields of include/tsd.h (parsed from the header), one per argument of
launch_flash_attention.  Operands are flat fp16 arrays in the device layout - Q [B][Sq][ldq], K [B][Sk][ldk], V^T [B][H*d][ldvt] - whose
pitch gaps hold the NaN pattern (an over-read shows as a non-finite output); V^T columns [Sk, Skv), Skv = min(round_up(Sk, 8), ldvt),
are the pad columns the last key tile streams and hold what `pack(..., pad=)` puts there.

Reference (`reference`), float64 on the fp16 input bits, per batch and head:  o = softmax_k(scale q.k) v.

Bound (second value of `reference`): |y - o| <= bound for EVERY output element, a function of the inputs alone.  Units: scores are in
log2 units, t_k = c q.k with c = scale log2(e); u = 2^-24 (fp32), h = 2^-11 (fp16); w_k = the reference's softmax weights.
  * Q rounding.  The kernel multiplies q_i by the fp32 constant c in fp32 and rounds once to fp16: |dq_i| <= |q_i c| (h + 2^-22) (the
    2^-22 covers the rounding of c itself and of the fp32 product), 2^-25 absolute below the fp16 normals, 0 for q_i = 0.  Through
    sum_i |dq_i| |k_i| it moves key k's exponent by at most EQ_k.
  * QK^T accumulation.  fp32 accumulation over the padded depth dpad (48 / 80 / 160) with -ref as C operand (the 8-wave kernel: as the
    product of pad column 40), the tile-0 subtraction of the reference and its later moves: gamma_(dpad+3) (sum_i |q_i k_i| + EQ_k + 2 R)
    with R = (max_k |t_k| + HEADROOM + LAZY)(1 + 2^-10) - any reference the kernel can hold (the 8-wave kernel rounds it to 32 x fp16).
    E_k = EQ_k + this is the per-key exponent error.
  * v_exp_f32: 4 fp32 ulp (the project's 4x convention over the 1 ulp of AMD's ISA documentation): p~_k = P_k 2^(+-E_k) (1 +- 4u).
  * P rounding: one fp16 rounding, h relative.  rho_k = 2^E_k (1 + 4u)(1 + h) - 1 bounds the relative error of the rounded P upwards,
    rlo_k = 1 - 2^-E_k (1 - 4u)(1 - h) downwards.
      - d = 40, 80: the ones row sums the SAME rounded P as the numerator, so with P^_k = P_k (1 + r_k) + f_k the identity
        y - o = sum_k (P_k r_k + f_k)(v_kj - o_j) / sum_k P^_k holds exactly:  sum_k w_k rho_k |v_kj - o_j| / den.
      - d = 160: the denominator sums the unrounded p~: the rounding does not cancel, h sum_k w_k (1 + rho'_k) |v_kj| is added and rho' (no
        (1 + h) factor) replaces rho in the first term.
    den = 1 - sum_k w_k rlo_k - n_S floor (the smallest the device's row sum can be relative to the exact one).
  * subnormal floor of P: below 2^-14 (kernel units) the fp16 rounding error is 2^-25 absolute, f_k; the row sum is at least the largest P,
    2^-(HEADROOM + slack) in the optimistic pass and 1 in the exact pass, so floor = 2^-25 2^(4 + slack) ~ 2^-21 and the term is
    floor sum_{k in S} |v_kj - o_j| (d = 160: |v_kj|), S = keys more than 10 - slack - E_k log2 units below the row maximum - the only
    keys whose P can be subnormal under any reference the kernel can hold; slack = the 8-wave kernel's reference rounding.
  * P.V accumulation, reference moves, normalisation: fp32 accumulation over 64 ntiles keys in numerator and denominator, one fp32
    rounding per move (at most one per tile) in each, the reciprocal (4u) and the product (u):
    (gamma_n + 5u)(amp sum_k w_k |v_kj| + |o_j| + e), n = 65 ntiles + 2, amp = (1 + max rho) / den, e = the terms above.
  * output rounding: h (|o_j| + e32) + 2^-25.
`well_conditioned` (inputs only) is true when every rho_k <= 1/4; every sweep case but `onehot` asserts it.  The bound gets its teeth
from the seeded defects of `emulate` (tests/test_attn_ref_cpu.py), not from a chosen fraction of the signal.

`predict_repeat` says per workgroup whether the optimistic pass must, must not or may overflow (an fp16 P >= 65520, i.e. an exponent of
log2(65520) = 15.99965 above the optimistic reference max(tile-0 maximum, own-block maximum) + HEADROOM), from the exact scores with a
margin of E_k on both scores involved plus the 8-wave kernel's reference rounding.

`emulate` restates the device arithmetic in numpy float32: fp16 Q after the fp32 multiply, fp32 scores, the optimistic reference with
the own-block maximum, fp16 P, the ones-row sum (d = 40, 80) or the fp32 sum of the unrounded P (d = 160), the exact repeat per
workgroup with LAZY reference moves decided per wave (32 / 64 rows), fp16 output - with seeded defects (`MUTATIONS`).

Row softmax: `softmax_reference` (fp64 on the input bits, its bound: __expf is exp2 of a rounded product, (2 |x - m| + 4) u relative -
3 |x - m| for fp32 inputs, whose difference rounds too -, the fp32 sum, reciprocal and product, then h and the 2^-25 floor for fp16
output; columns [kept, zero_to) of the causal form are exact zeros) and `softmax_emulate`.
"""
import functools
import math
import numpy as np

import replay
from replay import NAN16, NAN32, bits_f32, f32_bits

U32 = 2.0 ** -24
H16 = 2.0 ** -11
LOG2E = 1.4426950408889634
HEADROOM, LAZY = 4.0, 12.0          # TSD_ATTN_HEADROOM, TSD_ATTN_LAZY (csrc/attn_common.h)
OVERFLOW = math.log2(65520.0)       # the smallest exponent whose fp16 P is infinite
EXP_ULPS = 4.0


def _parse():
    txt = replay.header()
    return replay.enums(txt, {"TSD_AD_": "tsd_attn_desc_field", "TSD_AO_": "tsd_attn_operand", "TSD_AI_": "tsd_attn_info",
                              "TSD_AM_": "tsd_attn_mode", "TSD_AK_": "tsd_attn_kernel"}) + [replay.version(txt, "TSD_AD_VERSION_1")]


AD, AO, AI, AM, AK, AD_VERSION = _parse()
COUNT = AD["COUNT"]
INPUTS = ("Q", "K", "VT", "X")
KERNEL_NAME = {v: k for k, v in AK.items()}
WG_ROWS = {AK["40_1"]: 128, AK["40_2"]: 256, AK["40_8W"]: 512, AK["80"]: 128, AK["160"]: 128}
WAVE_ROWS = {AK["40_1"]: 32, AK["40_2"]: 64, AK["40_8W"]: 64, AK["80"]: 32, AK["160"]: 32}
SOFTMAX_KERNEL = {"f32": 1, "generic": 2, "h8_1": 3, "h8_2": 4}


def round_up(a, b):
    return (a + b - 1) // b * b


def F(d, k):
    return int(d[AD[k]])


def attn_desc(B, H, d, Sq, Sk, kernel=0, diag=1, scale=None, ldq=None, ldk=None, ldvt=None, ldo=None, gap=16, dense=False):
    """Pitches H*d + 8, V^T pitch round_up(Sk, 8) + 8 and batch strides with a gap of `gap` elements unless given (dense: none)."""
    C = H * d
    e = 0 if dense else 8
    ldq, ldk, ldo = ldq or C + e, ldk or C + e, ldo or C + e
    ldvt = ldvt or round_up(max(Sk, 1), 8) + e
    g = 0 if dense else gap
    desc = np.zeros(COUNT, np.int64)
    for k, v in dict(VERSION=AD_VERSION, MODE=AM["ATTN"], B=B, H=H, D=d, SQ=Sq, SK=Sk, LDQ=ldq, LDK=ldk, LDVT=ldvt, LDO=ldo,
                     SQB=max(Sq, 1) * ldq + g, SKB=max(Sk, 1) * ldk + g, SVTB=C * ldvt + g, SOB=max(Sq, 1) * ldo + g,
                     SCALE=f32_bits(1.0 / math.sqrt(d) if scale is None else scale), KERNEL=kernel, DIAG=diag).items():
        desc[AD[k]] = int(v)
    return desc


def softmax_desc(rows, cols, ld=None, dtype=1, causal=0, zero_to=0):
    desc = np.zeros(COUNT, np.int64)
    for k, v in dict(VERSION=AD_VERSION, MODE=AM["SOFTMAX_ROWS"], ROWS=rows, COLS=cols, LD=ld or cols, DTYPE=dtype, CAUSAL=causal,
                     ZERO_TO=zero_to).items():
        desc[AD[k]] = int(v)
    return desc


def scale_of(d):
    return bits_f32(F(d, "SCALE"))


def skv_of(d):
    return min(round_up(max(F(d, "SK"), 1), 8), F(d, "LDVT"))


def dtype_of(s, d):
    return np.float32 if F(d, "MODE") == AM["SOFTMAX_ROWS"] and F(d, "DTYPE") == 0 and s in ("X", "O") else np.float16


def extents(d):
    """Elements of every operand slot (0 = unused): what the entry's sizing-only mode must return."""
    e = dict.fromkeys(INPUTS + ("O",), 0)
    if F(d, "MODE") == AM["ATTN"]:
        B, C, Sq, Sk = F(d, "B"), F(d, "H") * F(d, "D"), max(F(d, "SQ"), 1), max(F(d, "SK"), 1)
        e["Q"] = (B - 1) * F(d, "SQB") + (Sq - 1) * F(d, "LDQ") + C
        e["K"] = (B - 1) * F(d, "SKB") + (Sk - 1) * F(d, "LDK") + C
        e["VT"] = (B - 1) * F(d, "SVTB") + (C - 1) * F(d, "LDVT") + skv_of(d)
        e["O"] = (B - 1) * F(d, "SOB") + (Sq - 1) * F(d, "LDO") + C
    else:
        e["X"] = e["O"] = (F(d, "ROWS") - 1) * F(d, "LD") + max(F(d, "COLS"), F(d, "ZERO_TO"))
    return e


def plan(d, attn_qb=2, attn_wg8=1, attn_xcd=0):
    """launch_flash_attention's dispatch (attn_plan, csrc/kernels_attn.hip) restated: kernel, diag and xcd_map under the default options."""
    B, H, hd, Sq, Sk, force = F(d, "B"), F(d, "H"), F(d, "D"), F(d, "SQ"), F(d, "SK"), F(d, "KERNEL")
    p = dict(DIAG=1 if F(d, "DIAG") and Sq == Sk else 0, XCD_MAP=1 if attn_xcd and (B * H) % 8 == 0 and Sk >= 512 else 0)
    if hd == 40:
        if (force == 3) if force else (attn_wg8 and Sk >= 512 and -(-Sq // 512) * H >= 64):
            p["KERNEL"] = AK["40_8W"]
        elif (force == 2) if force else (attn_qb == 2 and Sk >= 512 and -(-Sq // 256) * H >= 64):
            p["KERNEL"] = AK["40_2"]
        else:
            p["KERNEL"] = AK["40_1"]
    else:
        p["KERNEL"] = {80: AK["80"], 160: AK["160"]}[hd]
    return p


# ---- operands in the device layout ---------------------------------------------------------------------------------------------------
def _h(x):
    return np.asarray(x, np.float64).astype(np.float16)


def pack(d, q, k, v, pad=0.0):
    """q [B][H][Sq][d], k, v [B][H][Sk][d] -> {Q, K, VT} flat fp16 in the device layout.  Pitch gaps and V^T columns >= Skv hold the NaN
    pattern; V^T columns [Sk, Skv) hold `pad` (a scalar, or an array broadcast over [B][H*d][Skv - Sk])."""
    B, H, hd, Sq, Sk = F(d, "B"), F(d, "H"), F(d, "D"), F(d, "SQ"), F(d, "SK")
    ext, C, Skv = extents(d), H * hd, skv_of(d)
    ops = {s: np.full(ext[s], NAN16, np.float16) for s in ("Q", "K", "VT")}
    for name, x, S, ld, sb in (("Q", q, Sq, F(d, "LDQ"), F(d, "SQB")), ("K", k, Sk, F(d, "LDK"), F(d, "SKB"))):
        x = _h(x).transpose(0, 2, 1, 3).reshape(B, S, C)
        idx = (np.arange(B)[:, None, None] * sb + np.arange(S)[None, :, None] * ld + np.arange(C)[None, None, :])
        ops[name][idx.ravel()] = x.ravel()
    vt = np.empty((B, C, Skv), np.float16)
    vt[:, :, :Sk] = _h(v).transpose(0, 1, 3, 2).reshape(B, C, Sk)
    if Skv > Sk:
        vt[:, :, Sk:] = _h(np.broadcast_to(pad, (B, C, Skv - Sk)))
    idx = np.arange(B)[:, None, None] * F(d, "SVTB") + np.arange(C)[None, :, None] * F(d, "LDVT") + np.arange(Skv)[None, None, :]
    ops["VT"][idx.ravel()] = vt.ravel()
    return ops


def unpack_inputs(d, ops):
    """-> q [B][H][Sq][d], k, v [B][H][Sk][d], vpad [B][H][Skv - Sk][d] (fp16)."""
    B, H, hd, Sq, Sk = F(d, "B"), F(d, "H"), F(d, "D"), F(d, "SQ"), F(d, "SK")
    C, Skv = H * hd, skv_of(d)
    out = []
    for name, S, ld, sb in (("Q", Sq, F(d, "LDQ"), F(d, "SQB")), ("K", Sk, F(d, "LDK"), F(d, "SKB"))):
        idx = (np.arange(B)[:, None, None] * sb + np.arange(S)[None, :, None] * ld + np.arange(C)[None, None, :])
        out.append(ops[name][idx].reshape(B, S, H, hd).transpose(0, 2, 1, 3))
    idx = np.arange(B)[:, None, None] * F(d, "SVTB") + np.arange(C)[None, :, None] * F(d, "LDVT") + np.arange(Skv)[None, None, :]
    vt = ops["VT"][idx].reshape(B, H, hd, Skv).transpose(0, 1, 3, 2)
    return out[0], out[1], vt[:, :, :Sk], vt[:, :, Sk:]


def o_index(d):
    B, H, hd, Sq = F(d, "B"), F(d, "H"), F(d, "D"), F(d, "SQ")
    return (np.arange(B)[:, None, None] * F(d, "SOB") + np.arange(Sq)[None, :, None] * F(d, "LDO") + np.arange(H * hd)[None, None, :])


def unpack_output(d, o):
    """flat O -> [B][H][Sq][d]."""
    B, H, hd, Sq = F(d, "B"), F(d, "H"), F(d, "D"), F(d, "SQ")
    return np.asarray(o)[o_index(d)].reshape(B, Sq, H, hd).transpose(0, 2, 1, 3)


def pack_output(d, y):
    """[B][H][Sq][d] -> flat O with the NaN pattern in the gaps (what the entry returns for a launch that wrote exactly its elements)."""
    B, H, hd, Sq = F(d, "B"), F(d, "H"), F(d, "D"), F(d, "SQ")
    o = np.full(extents(d)["O"], NAN16, np.float16)
    o[o_index(d).ravel()] = np.asarray(y, np.float16).transpose(0, 2, 1, 3).reshape(B, Sq, H * hd).ravel()
    return o


# ---- reference and bound ---------------------------------------------------------------------------------------------------------
def _gamma(n):
    return n * U32 / (1.0 - n * U32)


def _head_terms(d, kern, q, k):
    """Exact scores and their error terms for one (batch, head): T, E [Sq][Sk] (log2 units), slack (reference rounding, per row)."""
    hd = F(d, "D")
    c = scale_of(d) * LOG2E
    qc = q * c
    dq = np.where(qc == 0.0, 0.0, np.maximum(np.abs(qc) * (H16 + 2.0 ** -22), 2.0 ** -25))
    ak = np.abs(k)
    T = qc @ k.T
    A = np.abs(qc) @ ak.T
    EQ = dq @ ak.T
    R = (np.abs(T).max(axis=1, keepdims=True) + HEADROOM + LAZY) * (1.0 + 2.0 ** -10)
    E = EQ + _gamma(round_up(hd, 16) + 3) * (A + EQ + 2.0 * R)
    m = T.max(axis=1)
    slack = (np.maximum(H16 * (np.abs(m) + HEADROOM + E.max(axis=1)), 0.0625) if kern == AK["40_8W"] else np.zeros_like(m)) + 3 * U32 * R[:, 0]
    return T, E, slack


def _rho(E, rounded=True):
    hh = H16 if rounded else 0.0
    return np.exp2(E) * (1 + EXP_ULPS * U32) * (1 + hh) - 1.0, 1.0 - np.exp2(-E) * (1 - EXP_ULPS * U32) * (1 - hh)


def well_conditioned(d, ops):
    q, k, _, _ = (x.astype(np.float64) for x in unpack_inputs(d, ops))
    kern = plan(d)["KERNEL"]
    return all(_rho(_head_terms(d, kern, q[b, h], k[b, h])[1])[0].max() <= 0.25 for b in range(q.shape[0]) for h in range(q.shape[1]))


def reference(d, ops, kernel=None):
    """-> (o, bound) [B][H][Sq][d] float64."""
    q, k, v, _ = (x.astype(np.float64) for x in unpack_inputs(d, ops))
    B, H, Sq, hd = q.shape
    Sk = k.shape[2]
    kern = kernel or plan(d)["KERNEL"]
    ones_row = hd != 160
    ntiles = -(-Sk // 64)
    g_acc = _gamma(65 * ntiles + 2) + 5 * U32
    o = np.empty((B, H, Sq, hd))
    bound = np.empty_like(o)
    for b in range(B):
        for h in range(H):
            T, E, slack = _head_terms(d, kern, q[b, h], k[b, h])
            m = T.max(axis=1, keepdims=True)
            w = np.exp2(T - m)
            w /= w.sum(axis=1, keepdims=True)
            vv = v[b, h]
            oo = w @ vv
            rho, rlo = _rho(E, rounded=ones_row)
            inS = (T < m - (10.0 - slack[:, None] - E)).astype(np.float64)
            floor = 2.0 ** -25 * np.exp2(HEADROOM + slack)[:, None]
            den = 1.0 - (w * rlo).sum(axis=1, keepdims=True) - inS.sum(axis=1, keepdims=True) * floor
            den = np.where(den > 0, den, np.nan)       # no bound can be given: the comparison fails
            wr = w * rho
            wv = w @ np.abs(vv)
            e = np.empty((Sq, hd))
            for j in range(hd):
                if ones_row:
                    dev = np.abs(vv[None, :, j] - oo[:, j:j + 1])
                    e[:, j] = (wr * dev).sum(axis=1) + floor[:, 0] * (inS * dev).sum(axis=1)
                else:
                    dev = np.abs(vv[None, :, j] - oo[:, j:j + 1])
                    av = np.abs(vv[None, :, j])
                    e[:, j] = (wr * dev).sum(axis=1) + H16 * (w * (1 + rho) * av).sum(axis=1) + floor[:, 0] * (inS * av).sum(axis=1)
            e /= den
            amp = (1.0 + rho.max(axis=1, keepdims=True)) / den
            e32 = e + g_acc / (1 - g_acc) * (amp * wv + np.abs(oo) + e)
            o[b, h] = oo
            bound[b, h] = e32 + H16 * (np.abs(oo) + e32) + 2.0 ** -25
    return o, bound


def predict_repeat(d, ops, kernel=None):
    """Per workgroup [B*H][ceil(Sq / rows)]: +1 the optimistic pass must overflow (exact repeat), -1 it must not, 0 either."""
    q, k, _, _ = (x.astype(np.float64) for x in unpack_inputs(d, ops))
    B, H, Sq, hd = q.shape
    Sk = k.shape[2]
    p = plan(d)
    kern = kernel or p["KERNEL"]
    rows = WG_ROWS[kern]
    out = np.zeros((B * H, -(-Sq // rows)), np.int64)
    for b in range(B):
        for h in range(H):
            T, E, slack = _head_terms(d, kern, q[b, h], k[b, h])
            t0 = min(64, Sk)
            lo, hi = (T - E)[:, :t0].max(axis=1), (T + E)[:, :t0].max(axis=1)     # the computed tile-0 maximum lies in [lo, hi]
            if p["DIAG"]:
                own = np.minimum((np.arange(Sq)[:, None] // 32) * 32 + np.arange(32)[None, :], Sk - 1)
                r = np.arange(Sq)[:, None]
                lo = np.maximum(lo, (T - E)[r, own].max(axis=1))
                hi = np.maximum(hi, (T + E)[r, own].max(axis=1))
            must = ((T - E) - (hi + HEADROOM + slack)[:, None] >= OVERFLOW + 1e-5).any(axis=1)
            mustnot = ((T + E) - (lo + HEADROOM - slack)[:, None] <= OVERFLOW - 1e-5).all(axis=1)
            for g in range(out.shape[1]):
                sl = slice(g * rows, min((g + 1) * rows, Sq))
                out[b * H + h, g] = 1 if must[sl].any() else (-1 if mustnot[sl].all() else 0)
    return out


def check(d, ops, out, kernel=None, ref=None):
    """Every element of the flat output against the bound -> (failures, worst error / bound)."""
    o, bd = ref if ref is not None else reference(d, ops, kernel)
    y = unpack_output(d, out).astype(np.float64)
    fails = []
    if not np.isfinite(y).all():
        fails.append(f"{int((~np.isfinite(y)).sum())} non-finite outputs")
    if not np.isfinite(bd).all():
        fails.append("no bound can be given for some rows (the row sum may vanish)")
    err = np.abs(np.where(np.isfinite(y), y, 0.0) - o)
    ratio = np.where(np.isfinite(bd), err / np.where(np.isfinite(bd), bd, 1.0), np.inf)
    worst = float(ratio.max())
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        fails.append(f"{int((ratio > 1).sum())} of {ratio.size} elements outside the bound; worst at [b,h,q,j] = {tuple(map(int, i))}: "
                     f"got {y[i]!r}, reference {o[i]!r}, bound {bd[i]:.3e}, ratio {worst:.3f}")
    return fails, worst


# ---- emulation of the device arithmetic -------------------------------------------------------------------------------------------
MUTATIONS = ("drop_last_key", "admit_masked_key", "scale_sqrt48", "v_swap_bits23", "head_offset_b", "no_alpha", "flush_subnormal_p",
             "sum_unrounded_p", "q_double_round", "clamp_zero_row", "pad_weight_2m24")


def _quant8(want):
    """The reference the 8-wave kernel can subtract: 32 x fp16, small ones snapped to 0."""
    q = (np.clip(want, -2.0e6, 2.0e6) * np.float32(1 / 32)).astype(np.float16).astype(np.float32) * np.float32(32)
    return np.where(np.abs(want) < 0.0625, np.float32(0), q).astype(np.float32)


def _p16(x, mut):
    p32 = np.exp2(x.astype(np.float32))
    with np.errstate(over="ignore"):
        p16 = p32.astype(np.float16)
    if mut == "flush_subnormal_p":
        p16 = np.where(np.abs(p16) < np.float16(2.0 ** -14), np.float16(0), p16)
    return p32, p16


def emulate(d, ops, mut=None, kernel=None):
    """-> (flat O as the entry would return it, workgroups that took the exact repeat)."""
    assert mut is None or mut in MUTATIONS, mut
    q, k, v, vpad = unpack_inputs(d, ops)
    B, H, Sq, hd = q.shape
    Sk, Skv = k.shape[2], skv_of(d)
    p = plan(d)
    kern = kernel or p["KERNEL"]
    rows_wg, rows_wave = WG_ROWS[kern], WAVE_ROWS[kern]
    ones_row = hd != 160
    sum_rounded = ones_row and not (mut == "sum_unrounded_p" and hd == 40)
    scale = np.float32(1.0 / math.sqrt(48.0)) if (mut == "scale_sqrt48" and hd == 40) else np.float32(scale_of(d))
    c = np.float32(scale * np.float32(LOG2E))
    ntiles = -(-Sk // 64)
    Kp, R = ntiles * 64, round_up(Sq, rows_wg)
    valid = np.arange(Kp) < Sk
    if Sk % 64:
        if mut == "drop_last_key":
            valid[Sk - 1] = False
        if mut == "admit_masked_key":
            valid[Sk] = True
    vperm = np.arange(Kp)
    if mut == "v_swap_bits23":
        vperm = (vperm & ~12) | ((vperm & 4) << 1) | ((vperm & 8) >> 1)
    y = np.zeros((B, H, Sq, hd), np.float16)
    repeats = 0
    NEG = np.float32(-1.0e30)
    for b in range(B):
        for h in range(H):
            hk = (h + 1) % H if (mut == "head_offset_b" and b > 0) else h
            qf = q[b, h].astype(np.float32)
            if mut == "q_double_round":
                qh = ((qf * scale).astype(np.float16).astype(np.float32) * np.float32(LOG2E)).astype(np.float16).astype(np.float32)
            else:
                qh = (qf * c).astype(np.float16).astype(np.float32)
            qr = np.concatenate([qh, np.zeros((R - Sq, hd), np.float32) if mut == "clamp_zero_row" else np.repeat(qh[-1:], R - Sq, axis=0)])
            kp = np.zeros((Kp, hd), np.float32)
            kp[:Sk] = k[b, hk].astype(np.float32)
            vp = np.zeros((Kp, hd), np.float32)
            vp[:Sk] = v[b, h].astype(np.float32)
            vp[Sk:Skv] = vpad[b, h].astype(np.float32)
            vp = vp[vperm]
            S = qr @ kp.T
            Sm = np.where(valid[None, :], S, NEG)
            mx = Sm[:, :64].max(axis=1)
            if p["DIAG"]:
                own = np.minimum((np.arange(R)[:, None] // 32) * 32 + np.arange(32)[None, :], Sk - 1)
                mx = np.maximum(mx, S[np.arange(R)[:, None], own].max(axis=1))
            want = (mx + np.float32(HEADROOM)).astype(np.float32)
            ref = _quant8(want) if kern == AK["40_8W"] else want
            X = np.where(valid[None, :], S - ref[:, None], NEG)
            p32, p16 = _p16(X, mut)
            if mut == "pad_weight_2m24":
                p16 = np.where(valid[None, :], p16, np.float16(2.0 ** -24))
                p32 = np.where(valid[None, :], p32, np.float32(2.0 ** -24))
            over = np.isinf(p16).any(axis=1).reshape(-1, rows_wg).any(axis=1)
            with np.errstate(invalid="ignore", over="ignore"):
                pf = p16.astype(np.float32)
                l = (pf if sum_rounded else p32).sum(axis=1, dtype=np.float32)
                O = np.where(np.isinf(pf), 0, pf) @ vp
            for g in np.nonzero(over)[0]:      # the exact repeat of workgroup g, reference moves decided per wave
                repeats += 1
                for r0 in range(g * rows_wg, (g + 1) * rows_wg, rows_wave):
                    sl = slice(r0, r0 + rows_wave)
                    m_run = np.zeros(rows_wave, np.float32)
                    oa = np.zeros((rows_wave, hd), np.float32)
                    la = np.zeros(rows_wave, np.float32)
                    for t in range(ntiles):
                        ks = slice(t * 64, t * 64 + 64)
                        s = np.where(valid[None, ks], S[sl, ks] - m_run[:, None], NEG)
                        mt = s.max(axis=1)
                        if t == 0 or (mt > LAZY).any():
                            delta = mt if t == 0 else np.maximum(mt, np.float32(0))
                            if kern == AK["40_8W"]:
                                delta = _quant8(m_run + delta) - m_run
                            m_run = m_run + delta
                            s = np.where(valid[None, ks], s - delta[:, None], NEG)
                            if t and mut != "no_alpha":
                                alpha = np.exp2(-delta).astype(np.float32)
                                oa *= alpha[:, None]
                                la *= alpha
                        e32, e16 = _p16(s, mut)
                        if mut == "pad_weight_2m24":
                            e16 = np.where(valid[None, ks], e16, np.float16(2.0 ** -24))
                            e32 = np.where(valid[None, ks], e32, np.float32(2.0 ** -24))
                        ef = e16.astype(np.float32)
                        oa += ef @ vp[ks]
                        la += (ef if sum_rounded else e32).sum(axis=1, dtype=np.float32)
                    O[sl], l[sl] = oa, la
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                y[b, h] = (O[:Sq] * (np.float32(1) / l[:Sq])[:, None]).astype(np.float16)
    return pack_output(d, y), repeats


# ---- inputs: the score shapes ------------------------------------------------------------------------------------------------------
KINDS = ("flat", "equal", "rising", "spike", "self_peaked", "low", "onehot", "subtail", "edge_lo", "edge_hi", "pbias", "qdouble")


def _unit(r, n, hd):
    """n directions of fp16-friendly entries, |u|^2 == 1 up to rounding."""
    u = r.standard_normal((n, hd))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _search_pbias(c):
    """An fp16 x > 0 such that, with q = x and k = -1 on one channel, P = 2^-(HEADROOM + fp16(x c)) rounds to fp16 with a relative error
    of at least +0.4 ulp (all such keys then carry the same positive rounding error: the rounded and unrounded row sums differ)."""
    xs = np.arange(0x3800, 0x4000, dtype=np.uint16).view(np.float16)          # 0.5 .. 2
    s = (xs.astype(np.float32) * np.float32(c)).astype(np.float16).astype(np.float64)
    p = np.exp2(-HEADROOM - s)
    rel = (p.astype(np.float16).astype(np.float64) - p) / p
    return float(xs[int(np.argmax(rel))]), float(rel.max())


def _search_qdouble(scale, c):
    """fp16 x+, x- in [1, 2) whose double rounding fp16(fp16(x scale) log2e) lies farthest above / below x c, in units of the allowance
    of the single rounding; -> (x+, ratio+, x-, ratio-)."""
    xs = np.arange(0x3C00, 0x4000, dtype=np.uint16).view(np.float16)
    x32 = xs.astype(np.float32)
    dbl = ((x32 * np.float32(scale)).astype(np.float16).astype(np.float32) * np.float32(LOG2E)).astype(np.float16).astype(np.float64)
    exact = xs.astype(np.float64) * c
    ratio = (dbl - exact) / (np.abs(exact) * (H16 + 2.0 ** -22))
    i, j = int(np.argmax(ratio)), int(np.argmin(ratio))
    return float(xs[i]), float(ratio[i]), float(xs[j]), float(ratio[j])


def make_inputs(d, kind="flat", seed=0, pad=0.0):
    """Operands of descriptor d with the score shape `kind` (K / Q scaling chosen here, never by random projections)."""
    B, H, hd, Sq, Sk = F(d, "B"), F(d, "H"), F(d, "D"), F(d, "SQ"), F(d, "SK")
    r = np.random.default_rng([seed, B, H, hd, Sq, Sk, KINDS.index(kind)])
    c = scale_of(d) * LOG2E
    q = r.standard_normal((B, H, Sq, hd))
    k = r.standard_normal((B, H, Sk, hd))
    v = r.standard_normal((B, H, Sk, hd))
    base = _unit(r, B * H, hd).reshape(B, H, 1, hd)
    ramp = np.arange(Sk).reshape(1, 1, Sk, 1) / max(Sk - 1, 1)
    if kind == "flat":
        pass
    elif kind == "equal":                      # every key equal: P = 2^-HEADROOM exactly, the output is the mean of V
        k = np.broadcast_to(k[:, :, :1], k.shape).copy()
    elif kind == "rising":                     # 0 .. 40 log2 units along the keys: exact repeat, found by the early look in long loops
        q = base * (1 + 0.05 * r.standard_normal((B, H, Sq, 1)))
        k = base * ramp * (40.0 / c) + 0.2 * k
    elif kind == "spike":                      # flat, one key of the last tile 30 units up: found by the final check
        q = base * 4 + 0.3 * q
        k = 0.3 * k
        k[:, :, Sk - 1] = base[:, :, 0] * (30.0 / (4 * c))
    elif kind == "self_peaked":                # every query's own key 60 units up
        u = _unit(r, B * H * Sq, hd).reshape(B, H, Sq, hd)
        q = u * 8
        k = (u * (60.0 / (8 * c)))[:, :, :Sk] if Sk <= Sq else k
    elif kind == "low":                        # all scores near -300
        q = base * 8 * (1 + 0.002 * r.standard_normal((B, H, Sq, 1)))
        k = -base * (300.0 / (8 * c)) + 0.1 * k
    elif kind == "onehot":                     # |q.k| scaled into the one-hot regime (exempt from well_conditioned)
        q = q * 24
    elif kind == "subtail":                    # key 0 at the maximum, the others 11 .. 30 units below; V of one sign
        q = base * 4 * (1 + 0.002 * r.standard_normal((B, H, Sq, 1)))
        x = np.concatenate([[0.0], np.linspace(11.0, 30.0, max(Sk - 1, 1))[:Sk - 1]]).reshape(1, 1, Sk, 1)
        k = -base * x / (4 * c)
        v = 0.5 + r.random((B, H, Sk, hd))
        v[:, :, 0] *= 0.25
    elif kind in ("edge_lo", "edge_hi"):       # tile 0 scores exactly 0 (reference = HEADROOM); rows whose later keys sit 15.5 .. 16.5 above it
        lv = np.array([15.5, 15.9] if kind == "edge_lo" else [15.5, 15.9, 16.1, 16.5]) + HEADROOM
        q = base * lv[np.arange(Sq) % len(lv)].reshape(1, 1, Sq, 1)
        k = np.zeros((B, H, Sk, hd))
        if Sk > 64:
            k[:, :, 64::7] = base / c
    elif kind == "pbias":                      # one hot channel: every key but key 0 carries the same P with the same rounding error
        x, _ = _search_pbias(np.float32(np.float32(scale_of(d)) * np.float32(LOG2E)))
        q = np.zeros((B, H, Sq, hd))
        q[..., 0] = x
        k = np.zeros((B, H, Sk, hd))
        k[:, :, 1:, 0] = -1.0
        v = 1.5 + np.round(r.random((B, H, 1, hd)) * 64) / 256 + np.zeros((B, H, Sk, hd))     # exactly representable, equal over the keys
    elif kind == "qdouble":                    # two key groups of equal score ~ 64 units on two channels, opposite V: a second rounding of
        xp, _, xm, _ = _search_qdouble(np.float32(scale_of(d)), c)    # Q moves the groups apart by more than one rounding per channel can
        q = np.zeros((B, H, Sq, hd))
        q[..., 0], q[..., 1] = xp, xm
        k = np.zeros((B, H, Sk, hd))
        k[:, :, 0::2, 0] = 64.0 / (xp * c)
        k[:, :, 1::2, 1] = 64.0 / (xm * c)
        v = np.where((np.arange(Sk) % 2 == 0).reshape(1, 1, Sk, 1), 1.0, -1.0) * (0.75 + 0.5 * r.random((B, H, Sk, hd)))
    else:
        raise ValueError(kind)
    return pack(d, q, k, v, pad)


KERNELS = (("40_1", 40, 1), ("40_2", 40, 2), ("40_8w", 40, 3), ("80", 80, 0), ("160", 160, 0))
SQ_SWEEP = (1, 31, 33, 128, 129, 257, 513)
SK_SWEEP = (1, 7, 8, 9, 63, 64, 65, 77, 129, 192, 193, 320, 576, 577, 1088, 1152)
PAD_SK = (7, 9, 77, 193)


def sweep():
    """[(name, descriptor, kind)] - the cases both tests/test_attn_ref_cpu.py (emulation) and tests/test_gpu_attn_ref.py (device) run."""
    out = []
    for kn, hd, mode in KERNELS:
        for Sq in (SQ_SWEEP if hd == 40 else (1, 33, 129)):
            out.append((f"{kn}/sq{Sq}", attn_desc(2, 2, hd, Sq, 77, kernel=mode), "flat"))
        for Sk in SK_SWEEP:
            out.append((f"{kn}/sk{Sk}", attn_desc(2, 2, hd, 33, Sk, kernel=mode), "flat"))
        for S in (33, 320, 577):
            for diag in (1, 0):
                out.append((f"{kn}/self{S}/diag{diag}", attn_desc(1, 1 if S > 320 else 2, hd, S, S, kernel=mode, diag=diag), "self_peaked"))
        for kind in ("equal", "rising", "spike", "low", "onehot", "subtail"):
            out.append((f"{kn}/{kind}", attn_desc(2, 1, hd, 65, 1152, kernel=mode), kind))
        for kind in ("edge_lo", "edge_hi"):
            out.append((f"{kn}/{kind}", attn_desc(1, 2, hd, 128, 129, kernel=mode), kind))
        out.append((f"{kn}/rising_partial", attn_desc(2, 2, hd, 33, 193, kernel=mode), "rising"))
        out.append((f"{kn}/pbias", attn_desc(1, 2, hd, 33, 320, kernel=mode), "pbias"))
        out.append((f"{kn}/qdouble", attn_desc(1, 2, hd, 33, 192, kernel=mode), "qdouble"))
    return out


def pad_sweep():
    """[(name, descriptor)]: partial last 8-column chunks of V^T; run with 0 and with +-60000 in columns [Sk, Skv)."""
    return [(f"{kn}/pad_sk{Sk}", attn_desc(2, 2, hd, 33, Sk, kernel=mode)) for kn, hd, mode in KERNELS for Sk in PAD_SK]


PAD_VALUE = 60000.0


def pad_fill(d):
    """+-60000 alternating over the V^T pad columns and channels."""
    C, n = F(d, "H") * F(d, "D"), skv_of(d) - F(d, "SK")
    return PAD_VALUE * np.where((np.arange(C)[:, None] + np.arange(n)[None, :]) % 2 == 0, 1.0, -1.0)[None]


@functools.lru_cache(maxsize=None)
def _case(name):
    _, d, kind = next(s for s in sweep() if s[0] == name)
    ops = make_inputs(d, kind, seed=7)
    return d, kind, ops, reference(d, ops)


def case(name):
    """(descriptor, kind, operands, (reference, bound)) of a sweep case - computed once per process, shared, never modified."""
    return _case(name)


# ---- row softmax -----------------------------------------------------------------------------------------------------------------
def softmax_kernel(d):
    if F(d, "DTYPE") == 0:
        return SOFTMAX_KERNEL["f32"]
    cols, ld = F(d, "COLS"), F(d, "LD")
    if F(d, "CAUSAL") == 0 and cols % 8 == 0 and ld % 8 == 0 and cols <= 4096:
        return SOFTMAX_KERNEL["h8_1"] if cols <= 2048 else SOFTMAX_KERNEL["h8_2"]
    return SOFTMAX_KERNEL["generic"]


def softmax_inputs(d, seed=0):
    """Rows of N(0, 2) scores, row 1 with a 60-unit spread; pitch gaps hold the NaN pattern."""
    rows, cols, ld = F(d, "ROWS"), F(d, "COLS"), F(d, "LD")
    dt = np.float16 if F(d, "DTYPE") else np.float32
    r = np.random.default_rng([seed, rows, cols, ld])
    x = 2.0 * r.standard_normal((rows, cols))
    if rows > 1:
        x[1] = np.linspace(-60.0, 0.0, cols)[r.permutation(cols)]
    flat = np.full(extents(d)["X"], NAN16 if dt == np.float16 else NAN32, dt)
    flat[(np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).ravel()] = x.astype(dt).ravel()
    return flat


def _softmax_rows_of(d, flat, width):
    rows, ld = F(d, "ROWS"), F(d, "LD")
    return np.asarray(flat)[np.arange(rows)[:, None] * ld + np.arange(width)[None, :]]


def softmax_kept(d):
    rows, cols, per = F(d, "ROWS"), F(d, "COLS"), F(d, "CAUSAL")
    return np.minimum(cols, np.arange(rows) % per + 1) if per > 0 else np.full(rows, cols)


def softmax_reference(d, x):
    """-> (y, bound) [rows][max(cols, zero_to)] float64; columns >= kept are 0 with bound 0."""
    rows, cols = F(d, "ROWS"), F(d, "COLS")
    width = max(cols, F(d, "ZERO_TO"))
    f16 = F(d, "DTYPE") == 1
    xs = _softmax_rows_of(d, x, cols).astype(np.float64)
    kept = softmax_kept(d)
    live = np.arange(cols)[None, :] < kept[:, None]
    xs = np.where(live, xs, -np.inf)
    m = xs.max(axis=1, keepdims=True)
    a = np.where(live, xs - m, 0.0)
    e = np.where(live, np.exp(a), 0.0)
    s = e.sum(axis=1, keepdims=True)
    y = e / s
    rk = ((2.0 if f16 else 3.0) * np.abs(a) + EXP_ULPS) * U32          # __expf: exp2 of the rounded product x log2(e)
    n = -(-cols // 256) + 24                                           # per-thread additions, the 6-step butterfly, the 4 wave sums
    rel = rk + (y * rk).sum(axis=1, keepdims=True) + _gamma(n) + 5 * U32
    e32 = y * rel * (1 + 1e-3)                                         # (second-order products of the relative terms)
    bound = e32 + (H16 * (y + e32) + 2.0 ** -25 if f16 else 0.0)
    out, bd = np.zeros((rows, width)), np.zeros((rows, width))
    out[:, :cols], bd[:, :cols] = y, np.where(live, bound, 0.0)
    return out, bd


SOFTMAX_MUTATIONS = ("causal_off_by_one", "exp2_without_log2e", "sum_skips_last_chunk")


def softmax_emulate(d, x, mut=None):
    """The kernels' arithmetic in float32 -> flat output in x's layout (untouched elements keep x / the NaN pattern)."""
    rows, cols, ld = F(d, "ROWS"), F(d, "COLS"), F(d, "LD")
    f16 = F(d, "DTYPE") == 1
    out = np.array(x, copy=True) if f16 else np.full(extents(d)["O"], NAN32, np.float32)
    kept = softmax_kept(d)
    if mut == "causal_off_by_one":
        kept = np.maximum(kept - 1, 1)
    xs = _softmax_rows_of(d, x, cols).astype(np.float32)
    for r in range(rows):
        n = int(kept[r])
        m = xs[r, :n].max()
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp2(((xs[r, :n] - m) * np.float32(1.0 if mut == "exp2_without_log2e" else LOG2E)).astype(np.float32)).astype(np.float32)
            s = (e[:max(n - n % 256, 1)] if mut == "sum_skips_last_chunk" else e).sum(dtype=np.float32)
            yr = (e * (np.float32(1) / s)).astype(out.dtype)
        out[r * ld:r * ld + n] = yr
        if F(d, "ZERO_TO") > n:
            out[r * ld + n:r * ld + F(d, "ZERO_TO")] = 0
    return out


def softmax_check(d, x, out, ref=None):
    y, bd = ref if ref is not None else softmax_reference(d, x)
    got = _softmax_rows_of(d, out, y.shape[1]).astype(np.float64)
    fails = []
    if not np.isfinite(got).all():
        fails.append(f"{int((~np.isfinite(got)).sum())} non-finite outputs")
    kept = softmax_kept(d)
    dead = np.arange(y.shape[1])[None, :] >= kept[:, None]
    if (np.where(dead, got, 0.0) != 0).any():
        fails.append("a column in [kept, zero_to) is not an exact zero")
    err = np.abs(np.where(np.isfinite(got), got, 0.0) - y)
    ratio = np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        fails.append(f"{int((ratio > 1).sum())} elements outside the bound; worst at {tuple(map(int, i))}: got {got[i]!r}, reference {y[i]!r}, "
                     f"bound {bd[i]:.3e}")
    return fails, worst


SOFTMAX_COLS = (8, 2040, 2048, 2056, 4096, 4104, 77)


def softmax_sweep():
    out = []
    for cols in SOFTMAX_COLS:
        out.append((f"f16/c{cols}", softmax_desc(3, cols, ld=cols + 8, dtype=1)))
        out.append((f"f32/c{cols}", softmax_desc(3, cols, ld=cols, dtype=0)))
    out.append(("f16/causal77", softmax_desc(3, 77, ld=88, dtype=1, causal=77, zero_to=80)))
    out.append(("f16/causal77_wrap", softmax_desc(80, 77, ld=88, dtype=1, causal=77, zero_to=80)))
    return out
