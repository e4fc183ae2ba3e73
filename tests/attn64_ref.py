"""fp64 reference, element-wise error bound, exact-repeat prediction and numpy emulation for the head-dimension-64 attention core,
flash_attn_kernel<64, 1> (csrc/kernels_attn.hip), reached through version-2 descriptors of tsd_debug_attn_run (test infrastructure).

Everything that does not depend on the head dimension is tests/attn_ref.py's: the descriptor fields, the device layout of the operands
(`pack`, `unpack_*`, `extents`), the score shapes (`make_inputs`), the per-key exponent error (`_head_terms`, fp32 accumulation over the
depth dpad = 64 - four 16-wide k-steps, none of them padded), `_rho`, `_gamma` and `check`.

What d = 64 shares with d = 160 and not with d = 40 / 80: the 32-row d blocks of V^T have no spare row, so there is no ones row and the
row sum is the fp32 sum of the UNROUNDED P.  The fp16 rounding of P then does not cancel between numerator and denominator, and the
bound is attn_ref's no-ones-row form (its docstring, "d = 160"), restated here as a function of the inputs alone:
    e_j = [ sum_k w_k rho'_k |v_kj - o_j|  +  h sum_k w_k (1 + rho'_k) |v_kj|  +  floor sum_{k in S} |v_kj| ] / den
with rho' the relative exponent error without the (1 + h) factor, den = 1 - sum_k w_k rlo_k - n_S floor, then the fp32 accumulation
over 64 ntiles keys, the reference moves, reciprocal and product ((gamma_(65 ntiles + 2) + 5u)(amp sum_k w_k |v_kj| + |o_j| + e_j)), and
the output rounding h (|o_j| + e32) + 2^-25.

What is new at d = 64 is the early look of the optimistic pass at an O accumulator (every TSD_ATTN_CHECK_EVERY = 8 key tiles).  It decides
what the check after the last tile decides, only sooner, so neither the repeat count nor a result depends on it: `predict_repeat` and
`emulate` know nothing of it, and the sweep holds the kernel to them on key loops where the look comes before the overflowing tile
(`spike_t9of10`: the final check must still find it), after it (`spike_t4of10`, `rising`) and not at all (fewer than nine tiles).
"""
import functools
import math

import numpy as np

import attn_ref as A
import replay
from attn_ref import F, AD, AO, AI, AK, INPUTS, U32, H16, HEADROOM, LAZY, OVERFLOW, LOG2E  # noqa: F401  (re-exported for the tests)

D = 64
AD_VERSION_2 = replay.version(replay.header(), "TSD_AD_VERSION_2")
AK64 = AK["64"]
WG_ROWS, WAVE_ROWS = 128, 32
CHECK_EVERY = 8         # TSD_ATTN_CHECK_EVERY (csrc/attn_common.h)


def attn_desc(B, H, Sq, Sk, hd=D, version=None, **kw):
    d = A.attn_desc(B, H, hd, Sq, Sk, **kw)
    d[AD["VERSION"]] = AD_VERSION_2 if version is None else version
    return d


def plan(d, attn_xcd=0):
    """attn_plan (csrc/kernels_attn.hip) at d = 64: one kernel at every shape."""
    B, H, Sq, Sk = F(d, "B"), F(d, "H"), F(d, "SQ"), F(d, "SK")
    assert F(d, "D") == D
    return dict(DIAG=1 if F(d, "DIAG") and Sq == Sk else 0, XCD_MAP=1 if attn_xcd and (B * H) % 8 == 0 and Sk >= 512 else 0, KERNEL=AK64)


def well_conditioned(d, ops):
    q, k, _, _ = (x.astype(np.float64) for x in A.unpack_inputs(d, ops))
    return all(A._rho(A._head_terms(d, AK64, q[b, h], k[b, h])[1])[0].max() <= 0.25 for b in range(q.shape[0]) for h in range(q.shape[1]))


def reference(d, ops):
    """-> (o, bound) [B][H][Sq][64] float64: attn_ref's no-ones-row bound at dpad = 64."""
    q, k, v, _ = (x.astype(np.float64) for x in A.unpack_inputs(d, ops))
    B, H, Sq, hd = q.shape
    assert hd == D
    ntiles = -(-k.shape[2] // 64)
    g_acc = A._gamma(65 * ntiles + 2) + 5 * U32
    o = np.empty((B, H, Sq, hd))
    bound = np.empty_like(o)
    for b in range(B):
        for h in range(H):
            T, E, slack = A._head_terms(d, AK64, q[b, h], k[b, h])
            m = T.max(axis=1, keepdims=True)
            w = np.exp2(T - m)
            w /= w.sum(axis=1, keepdims=True)
            vv = v[b, h]
            av = np.abs(vv)
            oo = w @ vv
            rho, rlo = A._rho(E, rounded=False)
            inS = (T < m - (10.0 - slack[:, None] - E)).astype(np.float64)
            floor = 2.0 ** -25 * np.exp2(HEADROOM + slack)[:, None]
            den = 1.0 - (w * rlo).sum(axis=1, keepdims=True) - inS.sum(axis=1, keepdims=True) * floor
            den = np.where(den > 0, den, np.nan)       # no bound can be given: the comparison fails
            wr = w * rho
            e = np.empty((Sq, hd))
            for j in range(hd):
                dev = np.abs(vv[None, :, j] - oo[:, j:j + 1])
                e[:, j] = (wr * dev).sum(axis=1)
            e += H16 * ((w * (1 + rho)) @ av) + floor * (inS @ av)
            e /= den
            amp = (1.0 + rho.max(axis=1, keepdims=True)) / den
            e32 = e + g_acc / (1 - g_acc) * (amp * (w @ av) + np.abs(oo) + e)
            o[b, h] = oo
            bound[b, h] = e32 + H16 * (np.abs(oo) + e32) + 2.0 ** -25
    return o, bound


def predict_repeat(d, ops):
    """Per workgroup [B*H][ceil(Sq / 128)]: +1 the optimistic pass must overflow (exact repeat), -1 it must not, 0 either."""
    q, k, _, _ = (x.astype(np.float64) for x in A.unpack_inputs(d, ops))
    B, H, Sq, _ = q.shape
    Sk = k.shape[2]
    diag = plan(d)["DIAG"]
    out = np.zeros((B * H, -(-Sq // WG_ROWS)), np.int64)
    for b in range(B):
        for h in range(H):
            T, E, slack = A._head_terms(d, AK64, q[b, h], k[b, h])
            t0 = min(64, Sk)
            lo, hi = (T - E)[:, :t0].max(axis=1), (T + E)[:, :t0].max(axis=1)     # the computed tile-0 maximum lies in [lo, hi]
            if diag:
                own = np.minimum((np.arange(Sq)[:, None] // 32) * 32 + np.arange(32)[None, :], Sk - 1)
                r = np.arange(Sq)[:, None]
                lo = np.maximum(lo, (T - E)[r, own].max(axis=1))
                hi = np.maximum(hi, (T + E)[r, own].max(axis=1))
            must = ((T - E) - (hi + HEADROOM + slack)[:, None] >= OVERFLOW + 1e-5).any(axis=1)
            mustnot = ((T + E) - (lo + HEADROOM - slack)[:, None] <= OVERFLOW - 1e-5).all(axis=1)
            for g in range(out.shape[1]):
                sl = slice(g * WG_ROWS, min((g + 1) * WG_ROWS, Sq))
                out[b * H + h, g] = 1 if must[sl].any() else (-1 if mustnot[sl].all() else 0)
    return out


def check(d, ops, out, ref=None):
    return A.check(d, ops, out, ref=ref if ref is not None else reference(d, ops))


# ---- emulation of the device arithmetic -------------------------------------------------------------------------------------------
MUTATIONS = ("drop_last_key", "admit_masked_key", "scale_sqrt80", "v_swap_bits23", "head_offset_b", "no_alpha", "flush_subnormal_p",
             "pad_weight_2m24", "skip_repeat", "early_look_drops_tail")
# (attn_ref's `q_double_round` is no defect here: 1 / sqrt(64) is a power of two, so rounding q scale first and q scale log2(e) after gives
# the bits of the single rounding - the `qdouble` score shape stays in the sweep as an input, without a mutation of its own.)


def emulate(d, ops, mut=None):
    """-> (flat O as the entry would return it, workgroups that took the exact repeat).  float32 throughout: fp16 Q after the fp32
    multiply, fp32 scores, the optimistic reference with the own-block maximum, fp16 P into the P.V product, the fp32 sum of the unrounded
    P as the row sum, the exact repeat per 128-row workgroup with LAZY reference moves decided per 32-row wave, fp16 output."""
    assert mut is None or mut in MUTATIONS, mut
    q, k, v, vpad = A.unpack_inputs(d, ops)
    B, H, Sq, hd = q.shape
    Sk, Skv = k.shape[2], A.skv_of(d)
    diag = plan(d)["DIAG"]
    scale = np.float32(1.0 / math.sqrt(80.0)) if mut == "scale_sqrt80" else np.float32(A.scale_of(d))
    c = np.float32(scale * np.float32(LOG2E))
    ntiles = -(-Sk // 64)
    Kp, R = ntiles * 64, A.round_up(Sq, WG_ROWS)
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
            qh = (qf * c).astype(np.float16).astype(np.float32)
            qr = np.concatenate([qh, np.repeat(qh[-1:], R - Sq, axis=0)])
            kp = np.zeros((Kp, hd), np.float32)
            kp[:Sk] = k[b, hk].astype(np.float32)
            vp = np.zeros((Kp, hd), np.float32)
            vp[:Sk] = v[b, h].astype(np.float32)
            vp[Sk:Skv] = vpad[b, h].astype(np.float32)
            vp = vp[vperm]
            S = qr @ kp.T
            Sm = np.where(valid[None, :], S, NEG)
            mx = Sm[:, :64].max(axis=1)
            if diag:
                own = np.minimum((np.arange(R)[:, None] // 32) * 32 + np.arange(32)[None, :], Sk - 1)
                mx = np.maximum(mx, S[np.arange(R)[:, None], own].max(axis=1))
            ref = (mx + np.float32(HEADROOM)).astype(np.float32)
            X = np.where(valid[None, :], S - ref[:, None], NEG)
            p32, p16 = A._p16(X, "flush_subnormal_p" if mut == "flush_subnormal_p" else None)
            if mut == "pad_weight_2m24":
                p16 = np.where(valid[None, :], p16, np.float16(2.0 ** -24))
                p32 = np.where(valid[None, :], p32, np.float32(2.0 ** -24))
            if mut == "early_look_drops_tail" and ntiles > CHECK_EVERY:      # a look that ended the pass and kept its sums
                p16[:, CHECK_EVERY * 64:] = 0
                p32[:, CHECK_EVERY * 64:] = 0
            over = np.isinf(p16).any(axis=1).reshape(-1, WG_ROWS).any(axis=1)
            with np.errstate(invalid="ignore", over="ignore"):
                pf = p16.astype(np.float32)
                l = p32.sum(axis=1, dtype=np.float32)
                O = np.where(np.isinf(pf), 0, pf) @ vp
                if mut == "skip_repeat":
                    O = np.where(np.isinf(pf).any(axis=1)[:, None], np.float32(np.inf), O)
            for g in (() if mut == "skip_repeat" else np.nonzero(over)[0]):      # the exact repeat of workgroup g
                repeats += 1
                for r0 in range(g * WG_ROWS, (g + 1) * WG_ROWS, WAVE_ROWS):
                    sl = slice(r0, r0 + WAVE_ROWS)
                    m_run = np.zeros(WAVE_ROWS, np.float32)
                    oa = np.zeros((WAVE_ROWS, hd), np.float32)
                    la = np.zeros(WAVE_ROWS, np.float32)
                    for t in range(ntiles):
                        ks = slice(t * 64, t * 64 + 64)
                        s = np.where(valid[None, ks], S[sl, ks] - m_run[:, None], NEG)
                        mt = s.max(axis=1)
                        if t == 0 or (mt > LAZY).any():
                            delta = mt if t == 0 else np.maximum(mt, np.float32(0))
                            m_run = m_run + delta
                            s = np.where(valid[None, ks], s - delta[:, None], NEG)
                            if t and mut != "no_alpha":
                                alpha = np.exp2(-delta).astype(np.float32)
                                oa *= alpha[:, None]
                                la *= alpha
                        e32, e16 = A._p16(s, "flush_subnormal_p" if mut == "flush_subnormal_p" else None)
                        if mut == "pad_weight_2m24":
                            e16 = np.where(valid[None, ks], e16, np.float16(2.0 ** -24))
                            e32 = np.where(valid[None, ks], e32, np.float32(2.0 ** -24))
                        oa += e16.astype(np.float32) @ vp[ks]
                        la += e32.sum(axis=1, dtype=np.float32)
                    O[sl], l[sl] = oa, la
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                y[b, h] = (O[:Sq] * (np.float32(1) / l[:Sq])[:, None]).astype(np.float16)
    return A.pack_output(d, y), repeats


# ---- inputs and the sweep -----------------------------------------------------------------------------------------------------------
def make_inputs(d, kind="flat", seed=0, pad=0.0):
    """attn_ref's score shapes, plus `spike_t<i>of<n>`: flat scores and one key of key tile i (counted from 1) 30 log2 units up."""
    if not kind.startswith("spike_t"):
        return A.make_inputs(d, kind, seed, pad)
    tile, n = (int(x) for x in kind[len("spike_t"):].split("of"))
    B, H, hd, Sq, Sk = F(d, "B"), F(d, "H"), F(d, "D"), F(d, "SQ"), F(d, "SK")
    assert -(-Sk // 64) == n and 1 <= tile <= n
    r = np.random.default_rng([seed, B, H, hd, Sq, Sk, 1000 + tile])
    c = A.scale_of(d) * LOG2E
    base = A._unit(r, B * H, hd).reshape(B, H, 1, hd)
    q = base * 4 + 0.3 * r.standard_normal((B, H, Sq, hd))
    k = 0.3 * r.standard_normal((B, H, Sk, hd))
    v = r.standard_normal((B, H, Sk, hd))
    k[:, :, (tile - 1) * 64 + 5] = base[:, :, 0] * (30.0 / (4 * c))
    return A.pack(d, q, k, v, pad)


SQ_SWEEP = (1, 31, 32, 33, 127, 128, 129)
SK_SWEEP = (1, 4, 63, 64, 65, 77, 128, 129, 577, 641)     # 577, 641: a partial last tile behind the ninth - the early look runs
PAD_SK = (7, 9, 77, 193)


def sweep():
    """[(name, descriptor, kind)] - the cases both tests/test_sd2_cpu.py (emulation) and tests/test_gpu_attn64.py (device) run.  B = 2 with
    batch-stride gaps and pitches wider than H * 64 unless the case says otherwise (attn_ref.attn_desc's defaults)."""
    out = []
    for Sq in SQ_SWEEP:
        out.append((f"sq{Sq}", attn_desc(2, 5, Sq, 77), "flat"))
    for Sk in SK_SWEEP:
        out.append((f"sk{Sk}", attn_desc(2, 5, 33, Sk), "flat"))
    out.append(("h20/sq129_sk65", attn_desc(2, 20, 129, 65), "flat"))
    out.append(("h20/sq33_sk641", attn_desc(2, 20, 33, 641), "flat"))
    for S in (33, 320, 577):
        for diag in (1, 0):
            out.append((f"self{S}/diag{diag}", attn_desc(1, 1 if S > 320 else 2, S, S, diag=diag), "self_peaked"))
    for kind in ("equal", "rising", "spike", "low", "onehot", "subtail"):
        out.append((kind, attn_desc(2, 1, 65, 1152), kind))
    for kind in ("edge_lo", "edge_hi"):
        out.append((kind, attn_desc(1, 2, 128, 129), kind))
    out.append(("rising_partial", attn_desc(2, 2, 33, 193), "rising"))
    out.append(("pbias", attn_desc(1, 2, 33, 320), "pbias"))
    out.append(("qdouble", attn_desc(1, 2, 33, 192), "qdouble"))
    out.append(("spike_t9of10", attn_desc(2, 2, 129, 640), "spike_t9of10"))     # behind the only early look (after tile 8): final check
    out.append(("spike_t4of10", attn_desc(2, 2, 129, 640), "spike_t4of10"))     # in front of it: found early, same repeats
    return out


def pad_sweep():
    """[(name, descriptor)]: partial last 8-column chunks of V^T; run with 0 and with +-60000 in columns [Sk, Skv)."""
    return [(f"pad_sk{Sk}", attn_desc(2, 2, 33, Sk)) for Sk in PAD_SK]


@functools.lru_cache(maxsize=None)
def _case(name):
    _, d, kind = next(s for s in sweep() if s[0] == name)
    ops = make_inputs(d, kind, seed=7)
    return d, kind, ops, reference(d, ops)


def case(name):
    """(descriptor, kind, operands, (reference, bound)) of a sweep case - computed once per process, shared, never modified."""
    return _case(name)


# the six cases (and the seed of their inputs) whose output digests the jitter build must reproduce (tests/test_gpu_attn64.py)
JITTER_CASES = ("sq129", "sk641", "h20/sq33_sk641", "self577/diag0", "rising", "spike_t9of10")
