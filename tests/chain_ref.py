"""fp64 reference, float32 emulation, checks and sweeps for the fused attention-block kernels of csrc/kernels_chain.hip -
attn_chain_kernel<KIND_HEAD>, attn_chain_kernel<KIND_TAIL> and the two weight-stream packers - run through tsd_debug_chain_run (test
infrastructure).

A launch is a descriptor: the int64 TSD_CD_* fields of include/tsd.h (parsed from the header).  Operands are flat arrays in the device
layout (TSD_CO_*), fp16 unless a bias / statistics table; every pitch gap, every K row >= T and every V^T column >= round_up(T, 8) holds
the NaN pattern (an over-read shows as a non-finite output); V^T columns [T, round_up(T, 8)) hold `pad`.

`reference(d, ops)`: float64 on the input bits - the operation, not the kernel.
  tail:  tok2 = ao.Wso^T + bso + tok;  q = LN(tok2).Wq^T;  per head softmax_k(scale q.k).v over the sample's T keys;
         tok3 = tok2 + attn.Wco^T + bco;  (a, g) = LN(tok3).W1^T + b1;  tok4 = tok3 + (a gelu_tanh(g)).W2^T + b2;  out = x + tok4.Wout^T + bout
  head:  tok = GN(x).Wc^T + b_in with the GIVEN (mean, rstd) pairs per group of 10 channels;  q | k | v = LN(tok).Win^T from the unrounded
         tok;  vt transposed per sample.
  LN is (x - mu) / (sigma + eps) with the population sigma.

`emulate(d, ops, chunk, mut)`: the reference restated in float32 with the device's rounding points - every A operand rounded to fp16 (GN(x),
LN outputs, q (scale log2e), P, the attention output, the GEGLU activations, tok4), fp32 accumulation in k-chunks of `chunk`, scores through
exp2 against the exact row maximum, the row sum over the rounded P, an fp32 residual stream, fp16 outputs.  It follows the reference's
formulas, not the kernel's lane layout, and returns every output with its value before the last fp16 rounding.

`check(d, ops, outs, emu)`, per output (token-major [M][width]; V^T is transposed back, so a "row" is a token):
  1. every logical element finite, every pitch gap still the fill, CHANGED == 0;
  2. |y - ref| <= ulp16(ref) / 2 + K_ELEM r(row), r(row) = rms of (y32 - ref) over that row of the emulation;
  3. the rms of y - ref over the whole output, every row, every column and every 16-row x 20-column tile (a lane group's share of a wave)
     is at most L_* times the emulation's rms over the same elements;
  4. tail gn_part against fp64 sums of the DEVICE's returned out over 32 rows x 10 channels, gamma_320-relative to sum |f| and sum f^2 (320 fp32 terms
     in any order; the square of an fp16 value is exact in fp32): the statistics describe the rounded output and must be consistent
     with it whatever the output's own error is.

The limits are measured, not chosen.  The device differs from the emulation only in fp32-level details (accumulation order, v_exp / v_rcp,
the merge of the four LayerNorm partials), each of which moves some intermediate fp16 roundings - exactly what another `chunk` does to the
emulation.  K_ELEM = 2 x the largest excess (|y' - ref| - ulp16(ref) / 2) / r(row) of the emulation y' at chunk in {8, 64, 160, 320}
against chunk = 32, L_* = 1 + 3 x the largest relative difference of that statistic between those orders, over the whole sweep
(`measure_limits`; tests/test_chain_ref_cpu.py recomputes them and asserts that the emulation alone stays below HALF of each margin).
Measured on the sweep below (seed 7), figures rounded up to two digits: the largest excess is 5.2 (5.13 on head/group_means; 3.4 .. 5.0
elsewhere), so K_ELEM = 10.4; the spreads are 0.55 % for the whole output (L 1.017), 12 % for tiles (L 1.36), 34 % for rows (tail/peaked, where one rounding flip of q moves a
score by 2e-3 and most rows have a second key within 2 units of the best - the row at 34 % has no near-tie, its gap is 1.2; 6 .. 19 %
elsewhere) and 43 % for 64-element columns (tail/T80; 3 .. 29 % elsewhere) - for both of
these 1 + 3 x spread would pass 2, and no L may: L = 2.0, which still leaves the emulation below half of the margin.
The checks get their teeth from the seeded defects of `emulate` (`MUTATIONS`), each rejected on a named sweep case.
"""
import functools
import math

import numpy as np

import replay
from replay import NAN16, NAN32, bits_f32, f32_bits

U32 = 2.0 ** -24
LOG2E = 1.4426950408889634
ORDERS = (8, 64, 160, 320)         # the other accumulation orders the limits are measured at (the emulation itself runs at 32)

# ---- the measured limits (measure_limits(); recomputed by tests/test_chain_ref_cpu.py) ---------------------------------------------------
MEASURED_EXCESS = 5.2
MEASURED_SPREAD = {"whole": 0.0055, "rows": 0.34, "cols": 0.43, "tiles": 0.12}
K_ELEM = 2.0 * MEASURED_EXCESS
L_STAT = {k: min(1.0 + 3.0 * v, 2.0) for k, v in MEASURED_SPREAD.items()}       # no L may exceed 2


def _parse():
    txt = replay.header()
    return replay.enums(txt, {"TSD_CD_": "tsd_chain_desc_field", "TSD_CO_": "tsd_chain_operand", "TSD_CI_": "tsd_chain_info",
                              "TSD_CM_": "tsd_chain_mode"}) + [replay.version(txt, "TSD_CD_VERSION_1")]


CD, CO, CI, CM, CD_VERSION = _parse()
COUNT = CD["COUNT"]
_BY_SLOT = sorted((k for k in CO if k != "COUNT"), key=CO.get)
INPUTS = tuple(s for s in _BY_SLOT if CO[s] < CO["OUT"])
OUTPUTS = tuple(s for s in _BY_SLOT if CO[s] >= CO["OUT"])
F32_SLOTS = ("BSO", "BCO", "B1", "B2", "BOUT", "GN_STATS", "B_IN", "GN_PART")
C, HD, HEADS = 320, 40, 8


def round_up(a, b):
    return (a + b - 1) // b * b


def F(d, k):
    return int(d[CD[k]])


def is_tail(d):
    return F(d, "MODE") == CM["TAIL"]


def dtype_of(s, d=None):
    return np.float32 if s in F32_SLOTS else np.float16


def tail_desc(B, S, T=77, gn=0, ld=(320, 320, 320, 320), ldk=320, ldvt=None, gap=0, ldw=(320, 320, 320, 320, 1280, 320), scale=None,
              eps=1e-5, krows=None, **over):
    """ld = (ao, tok, x, out); ldw = (so, q, co, 1, 2, out); gap: elements between the samples of Kc and V^T; krows: K rows a sample's
    stride spans (rows >= T hold the fill)."""
    ldvt = ldvt or round_up(max(T, 1), 8)
    d = np.zeros(COUNT, np.int64)
    v = dict(VERSION=CD_VERSION, MODE=CM["TAIL"], B=B, S=S, T=T, C=C, D=HD, HEADS=HEADS, LD_AO=ld[0], LD_TOK=ld[1], LD_X=ld[2], LD_OUT=ld[3],
             LDK=ldk, SKB=max(krows or T, 1) * ldk + gap, LDVT=ldvt, SVTB=over.get("C", C) * ldvt + gap, SCALE=f32_bits(1.0 / math.sqrt(HD) if scale is None else scale),
             EPS=f32_bits(eps), GN=gn, LDW_SO=ldw[0], LDW_Q=ldw[1], LDW_CO=ldw[2], LDW_1=ldw[3], LDW_2=ldw[4], LDW_OUT=ldw[5])
    v.update(over)
    for k, x in v.items():
        d[CD[k]] = int(x)
    return d


def head_desc(B, S, ld_x=320, ld_tok=320, ld_qk=640, ld_vt=None, gap=0, ldw=(320, 320), eps=1e-5, **over):
    ld_vt = ld_vt or S
    d = np.zeros(COUNT, np.int64)
    v = dict(VERSION=CD_VERSION, MODE=CM["HEAD"], B=B, S=S, T=1, C=C, D=HD, HEADS=HEADS, LD_X=ld_x, LD_TOK=ld_tok, LD_QK=ld_qk, LD_VT=ld_vt,
             S_VT=over.get("C", C) * ld_vt + gap, EPS=f32_bits(eps), LDW_C=ldw[0], LDW_IN=ldw[1])
    v.update(over)
    for k, x in v.items():
        d[CD[k]] = int(x)
    return d


def tv_of(d):
    return min(round_up(max(F(d, "T"), 1), 8), F(d, "LDVT"))


def extents(d):
    """Elements of every operand slot (0 = unused): what the entry's sizing-only mode must return."""
    e = dict.fromkeys(INPUTS + OUTPUTS, 0)
    B, S, Cc = F(d, "B"), F(d, "S"), F(d, "C")
    M = B * S
    rows = lambda n, f, w: (n - 1) * F(d, f) + w
    if is_tail(d):
        Tk = max(F(d, "T"), 1)
        e["AO"], e["TOK"], e["X"], e["OUT"] = rows(M, "LD_AO", Cc), rows(M, "LD_TOK", Cc), rows(M, "LD_X", Cc), rows(M, "LD_OUT", Cc)
        e["KC"] = (B - 1) * F(d, "SKB") + rows(Tk, "LDK", Cc)
        e["VT"] = (B - 1) * F(d, "SVTB") + rows(Cc, "LDVT", tv_of(d))
        e["WSO"], e["WQ"], e["WCO"], e["WOUT"] = (rows(Cc, f, Cc) for f in ("LDW_SO", "LDW_Q", "LDW_CO", "LDW_OUT"))
        e["W1"], e["W2"] = rows(8 * Cc, "LDW_1", Cc), rows(Cc, "LDW_2", 4 * Cc)
        e["BSO"] = e["BCO"] = e["B2"] = e["BOUT"] = Cc
        e["B1"] = 8 * Cc
        if F(d, "GN"):
            e["GN_PART"] = B * (S // 32) * 32 * 2
    else:
        e["X"], e["HTOK"], e["QK"] = rows(M, "LD_X", Cc), rows(M, "LD_TOK", Cc), rows(M, "LD_QK", 2 * Cc)
        e["GN_STATS"] = B * 32 * 2
        e["WC"], e["WIN"], e["B_IN"] = rows(Cc, "LDW_C", Cc), rows(3 * Cc, "LDW_IN", Cc), Cc
        e["HVT"] = (B - 1) * F(d, "S_VT") + rows(Cc, "LD_VT", S)
    return e


# ---- operands in the device layout ---------------------------------------------------------------------------------------------------
def _layout(d):
    """{slot: (batch, stride, rows, pitch, width)} of every 2-D fp16 operand of d (batch 1 unless per sample)."""
    B, S = F(d, "B"), F(d, "S")
    M = B * S
    if is_tail(d):
        T = F(d, "T")
        return dict(AO=(1, 0, M, F(d, "LD_AO"), C), TOK=(1, 0, M, F(d, "LD_TOK"), C), X=(1, 0, M, F(d, "LD_X"), C), OUT=(1, 0, M, F(d, "LD_OUT"), C),
                    KC=(B, F(d, "SKB"), T, F(d, "LDK"), C), VT=(B, F(d, "SVTB"), C, F(d, "LDVT"), tv_of(d)),
                    WSO=(1, 0, C, F(d, "LDW_SO"), C), WQ=(1, 0, C, F(d, "LDW_Q"), C), WCO=(1, 0, C, F(d, "LDW_CO"), C),
                    W1=(1, 0, 8 * C, F(d, "LDW_1"), C), W2=(1, 0, C, F(d, "LDW_2"), 4 * C), WOUT=(1, 0, C, F(d, "LDW_OUT"), C))
    return dict(X=(1, 0, M, F(d, "LD_X"), C), HTOK=(1, 0, M, F(d, "LD_TOK"), C), QK=(1, 0, M, F(d, "LD_QK"), 2 * C),
                HVT=(B, F(d, "S_VT"), C, F(d, "LD_VT"), S), WC=(1, 0, C, F(d, "LDW_C"), C), WIN=(1, 0, 3 * C, F(d, "LDW_IN"), C))


def index(d, slot):
    """Flat indices [batch][rows][width] of the logical elements of a 2-D operand."""
    b, sb, r, ld, w = _layout(d)[slot]
    return np.arange(b)[:, None, None] * sb + np.arange(r)[None, :, None] * ld + np.arange(w)[None, None, :]


def pack(d, logical):
    """{slot: logical array} -> {slot: flat array in the device layout, the NaN pattern everywhere else}.  2-D operands are [rows][width]
    (KC / VT / HVT: [B][rows][width]); fp32 tables are flat."""
    ext, lay = extents(d), _layout(d)
    ops = {}
    for s, x in logical.items():
        if s in lay:
            flat = np.full(ext[s], NAN16, np.float16)
            flat[index(d, s).ravel()] = np.asarray(x, np.float64).astype(np.float16).ravel()
        else:
            flat = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32).ravel())
            assert flat.size == ext[s], s
        ops[s] = flat
    return ops


def unpack(d, ops):
    """{slot: flat} -> {slot: logical array} (fp16 / fp32 as stored), for the slots present."""
    lay = _layout(d)
    out = {}
    for s, flat in ops.items():
        if s in lay:
            x = np.asarray(flat)[index(d, s)]
            out[s] = x if lay[s][0] > 1 or s in ("KC", "VT", "HVT") else x[0]
        else:
            out[s] = np.asarray(flat)
    return out


def token_major(d, s, flat):
    """An output as [M][width]: V^T transposed back per sample."""
    x = unpack(d, {s: flat})[s]
    if s == "HVT":
        return np.ascontiguousarray(x.transpose(0, 2, 1).reshape(F(d, "B") * F(d, "S"), C))
    return x


def fp16_outputs(d):
    return ("OUT",) if is_tail(d) else ("HTOK", "QK", "HVT")


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def _ln64(x, eps):
    mu = x.mean(axis=-1, keepdims=True)
    return (x - mu) / (np.sqrt(((x - mu) ** 2).mean(axis=-1, keepdims=True)) + eps)


def _gelu_tanh(x):
    return x * (0.5 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))))


def reference(d, ops):
    """-> {output: [M][width] float64} (V^T token-major)."""
    L = {k: v.astype(np.float64) for k, v in unpack(d, {s: ops[s] for s in ops if s not in OUTPUTS}).items()}
    B, S, eps = F(d, "B"), F(d, "S"), float(bits_f32(F(d, "EPS")))
    if not is_tail(d):
        st = L["GN_STATS"].reshape(B, 32, 2)
        mean, rstd = (np.repeat(np.repeat(st[:, :, i], 10, axis=1), S, axis=0) for i in (0, 1))
        tok = ((L["X"] - mean) * rstd) @ L["WC"].T + L["B_IN"]
        qkv = _ln64(tok, eps) @ L["WIN"].T
        return {"HTOK": tok, "QK": qkv[:, :2 * C], "HVT": qkv[:, 2 * C:]}
    T, scale = F(d, "T"), float(bits_f32(F(d, "SCALE")))
    tok2 = L["AO"] @ L["WSO"].T + L["BSO"] + L["TOK"]
    q = _ln64(tok2, eps) @ L["WQ"].T
    attn = np.empty_like(q)
    for b in range(B):
        k, v = L["KC"][b], L["VT"][b][:, :T].T
        for h in range(HEADS):
            c = slice(h * HD, (h + 1) * HD)
            s = scale * (q[b * S:(b + 1) * S, c] @ k[:, c].T)
            w = np.exp(s - s.max(axis=1, keepdims=True))
            attn[b * S:(b + 1) * S, c] = (w / w.sum(axis=1, keepdims=True)) @ v[:, c]
    tok3 = tok2 + attn @ L["WCO"].T + L["BCO"]
    h1 = _ln64(tok3, eps) @ L["W1"].T + L["B1"]
    tok4 = tok3 + (h1[:, 0::2] * _gelu_tanh(h1[:, 1::2])) @ L["W2"].T + L["B2"]
    return {"OUT": L["X"] + tok4 @ L["WOUT"].T + L["BOUT"]}


# ---- emulation of the device arithmetic -------------------------------------------------------------------------------------------
MUTATIONS = ("drop_last_key", "admit_key_T", "mask_fragment4_only", "scale_without_log2e", "ln_per_column_wave", "ln_merge_without_between_term",
             "geglu_halves_swapped", "geglu_chunk_repeated", "no_b2", "b1_not_interleaved", "long_residual_from_tok", "context_of_sample_0",
             "wco_ktiles_3_4_swapped", "gn_slab_of_64_rows",
             "gn_group_of_20", "stats_of_sample_0", "k_from_wq", "v_rows_in_qk_order", "vt_second_tile_at_column_0")
f32 = np.float32


def _h(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, f32).astype(np.float16).astype(f32)


def _mm(a, w, chunk):
    """a [M][K] . w [N][K]^T, fp32 accumulation over k-chunks of `chunk`."""
    K = a.shape[1]
    acc = np.zeros((a.shape[0], w.shape[0]), f32)
    wt = np.ascontiguousarray(w.T)
    for k0 in range(0, K, chunk):
        acc += a[:, k0:k0 + chunk] @ wt[k0:k0 + chunk]
    return acc


def _ln32(v, eps, mut):
    """fp16((v - mean) rs), rs = 1 / (sqrt(M2 / C) + eps), in float32."""
    if mut == "ln_per_column_wave":
        w = v.reshape(v.shape[0], 4, 80)
        mu = w.mean(axis=2, keepdims=True, dtype=f32)
        var = ((w - mu) ** 2).mean(axis=2, keepdims=True, dtype=f32)
        return _h(((w - mu) * (f32(1) / (np.sqrt(var) + f32(eps)))).reshape(v.shape))
    mu = v.mean(axis=1, keepdims=True, dtype=f32)
    if mut == "ln_merge_without_between_term":
        w = v.reshape(v.shape[0], 4, 80)
        var = ((w - w.mean(axis=2, keepdims=True, dtype=f32)) ** 2).sum(axis=(1, 2), dtype=f32)[:, None] * f32(1.0 / C)
    else:
        var = ((v - mu) ** 2).mean(axis=1, keepdims=True, dtype=f32)
    return _h((v - mu) * (f32(1) / (np.sqrt(var) + f32(eps))))


def _gelu32(x):
    """x sigmoid(2u) through exp2, the device's form of the tanh GELU (the exponent overflows to inf on one side: 1 / inf = 0)."""
    k0 = f32(-2.0 * 0.7978845608028654 * LOG2E)
    with np.errstate(over="ignore"):
        t = np.exp2(x * (x * x * (k0 * f32(0.044715)) + k0)).astype(f32)
        return x * (f32(1) / (f32(1) + t))


def _qk_order(rho):
    ii, fn = rho & 15, rho >> 4
    return (ii >> 2) * 20 + fn * 4 + (ii & 3)


def emulate(d, ops, chunk=32, mut=None):
    """-> ({output: flat array as the entry would return it}, {fp16 output: [M][width] float32 before the last rounding})."""
    assert mut is None or mut in MUTATIONS, mut
    L = {k: v.astype(f32) for k, v in unpack(d, {s: ops[s] for s in ops if s not in OUTPUTS}).items()}
    B, S, eps = F(d, "B"), F(d, "S"), f32(bits_f32(F(d, "EPS")))
    M = B * S
    ext = extents(d)
    if not is_tail(d):
        st = L["GN_STATS"].reshape(B, 32, 2)
        if mut == "stats_of_sample_0":
            st = np.broadcast_to(st[:1], st.shape)
        grp = np.arange(C) // (20 if mut == "gn_group_of_20" else 10)
        mean, rstd = (np.repeat(st[:, grp, i], S, axis=0) for i in (0, 1))
        tok32 = _mm(_h((L["X"] - mean) * rstd), L["WC"], chunk) + L["B_IN"]
        a = _ln32(tok32, eps, mut)
        wq, wk, wv = L["WIN"][:C], L["WIN"][C:2 * C], L["WIN"][2 * C:]
        if mut == "k_from_wq":
            wk = wq
        if mut == "v_rows_in_qk_order":
            wv = wv[(np.arange(C) // 80) * 80 + _qk_order(np.arange(C) % 80)]
        y32 = {"HTOK": tok32, "QK": np.concatenate([_mm(a, wq, chunk), _mm(a, wk, chunk)], axis=1), "HVT": _mm(a, wv, chunk)}
        vt = _h(y32["HVT"]).reshape(B, S, C).transpose(0, 2, 1)
        if mut == "vt_second_tile_at_column_0" and S > 64:
            vt = np.concatenate([vt[:, :, S - 64:], np.full((B, C, S - 64), np.nan, f32)], axis=2)
        return pack(d, {"HTOK": _h(tok32), "QK": _h(y32["QK"]), "HVT": vt}), y32
    T = F(d, "T")
    qscale = f32(f32(bits_f32(F(d, "SCALE"))) * f32(1.0 if mut == "scale_without_log2e" else LOG2E))
    res = L["TOK"] + (_mm(L["AO"], L["WSO"], chunk) + L["BSO"])
    qa = _h(_mm(_ln32(res, eps, mut), L["WQ"], chunk) * qscale)
    valid = np.arange(80) < T
    if mut == "drop_last_key" and T > 1:
        valid[T - 1] = False
    if mut == "admit_key_T" and T < 80:
        valid[T] = True
    if mut == "mask_fragment4_only":
        valid[T:64] = True
    attn = np.empty((M, C), f32)
    Tv = tv_of(d)
    for b in range(B):
        bc = 0 if mut == "context_of_sample_0" else b
        kp, vp = np.zeros((80, C), f32), np.zeros((80, C), f32)     # K rows >= T are fetched as zeros; V^T chunks past Tv as well
        kp[:T] = L["KC"][bc]
        vp[:Tv] = L["VT"][bc].T
        for h in range(HEADS):
            c = slice(h * HD, (h + 1) * HD)
            s = np.where(valid[None, :], qa[b * S:(b + 1) * S, c] @ kp[:, c].T, f32(-1.0e30))
            p = np.where(valid[None, :], _h(np.exp2(s - s.max(axis=1, keepdims=True))), f32(0))
            attn[b * S:(b + 1) * S, c] = _h((p @ vp[:, c]) * (f32(1) / p.sum(axis=1, dtype=f32))[:, None])
    wco = L["WCO"]
    if mut == "wco_ktiles_3_4_swapped":
        wco = np.concatenate([wco[:, :96], wco[:, 128:160], wco[:, 96:128], wco[:, 160:]], axis=1)
    res = res + (_mm(attn, wco, chunk) + L["BCO"])
    a = _ln32(res, eps, mut)
    b1 = L["B1"]
    b1a, b1g = (b1[:4 * C], b1[4 * C:]) if mut == "b1_not_interleaved" else (b1[0::2], b1[1::2])
    ha, hg = _mm(a, L["W1"][0::2], chunk) + b1a, _mm(a, L["W1"][1::2], chunk) + b1g
    if mut == "geglu_halves_swapped":
        ha, hg = hg, ha
    act = _h(ha * _gelu32(hg))
    if mut == "geglu_chunk_repeated":
        act[:, 128:256] = act[:, 0:128]
    res = res + (_mm(act, L["W2"], chunk) + (f32(0) if mut == "no_b2" else L["B2"]))
    y32 = (L["TOK"] if mut == "long_residual_from_tok" else L["X"]) + (_mm(_h(res), L["WOUT"], chunk) + L["BOUT"])
    outs = pack(d, {"OUT": _h(y32)})
    if F(d, "GN"):
        f = _h(y32).reshape(B, S // 32, 32, 32, 10)
        part = np.stack([f.sum(axis=(2, 4), dtype=f32), (f * f).sum(axis=(2, 4), dtype=f32)], axis=-1)      # [B][S/32][32][2]
        if mut == "gn_slab_of_64_rows":
            bad = np.full_like(part, NAN32)
            bad[:, :S // 64] = part[:, 1::2]          # both slabs of a workgroup land on slab (row / 64): the second one stays
            part = bad
        outs["GN_PART"] = np.ascontiguousarray(part.ravel())
    return outs, {"OUT": y32}


# ---- checks --------------------------------------------------------------------------------------------------------------------------
def ulp16(x):
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14))) - 10)


def _rms(e, axis=None):
    return np.sqrt((e * e).mean(axis=axis))


def _stats(err):
    """The rms of an error array [M][W] over the whole output, every row, every column and every 16 x 20 tile."""
    M, W = err.shape
    t = err.reshape(M // 16, 16, W // 20, 20)
    return {"whole": np.array([_rms(err)]), "rows": _rms(err, 1), "cols": _rms(err, 0), "tiles": np.sqrt((t * t).mean(axis=(1, 3))).ravel()}


def excess(y, ref, r_row):
    """(|y - ref| - ulp16(ref) / 2) / r(row), element-wise."""
    return (np.abs(y - ref) - ulp16(ref) / 2) / r_row[:, None]


def gn_part_check(d, out_flat, part_flat):
    """The statistics against fp64 sums of the rounded output they describe -> worst error / tolerance (inf: a non-finite entry)."""
    B, S = F(d, "B"), F(d, "S")
    f = unpack(d, {"OUT": out_flat})["OUT"].astype(np.float64).reshape(B, S // 32, 32, 32, 10)
    got = np.asarray(part_flat, np.float64).reshape(B, S // 32, 32, 2)
    if not np.isfinite(got).all() or not np.isfinite(f).all():
        return np.inf
    g = 320 * U32 / (1 - 320 * U32)
    e1 = np.abs(got[..., 0] - f.sum(axis=(2, 4))) / (g * np.abs(f).sum(axis=(2, 4)) + 1e-30)
    e2 = np.abs(got[..., 1] - (f * f).sum(axis=(2, 4))) / (g * (f * f).sum(axis=(2, 4)) + 1e-30)
    return float(max(e1.max(), e2.max()))


def check(d, ops, outs, emu, ref=None, changed=0, k_elem=None, l_stat=None):
    """outs: {output: flat array} as returned by the entry (or by `emulate`); emu: the result of `emulate(d, ops)`.
    -> (failures, {kind of check: worst ratio to its limit})."""
    k_elem, l_stat = K_ELEM if k_elem is None else k_elem, L_STAT if l_stat is None else l_stat
    ref = ref if ref is not None else reference(d, ops)
    e_out, e32 = emu
    fails, worst = [], dict.fromkeys(("elem",) + tuple(l_stat), 0.0)
    if changed:
        fails.append(f"{changed} guard / pitch-gap elements written")
    for s in fp16_outputs(d):
        flat = np.asarray(outs[s])
        gap = np.ones(flat.size, bool)
        gap[index(d, s).ravel()] = False
        if not (flat.view(np.uint16)[gap] == NAN16.view(np.uint16)).all():
            fails.append(f"{s}: a pitch gap was written")
        y = token_major(d, s, flat).astype(np.float64)
        if not np.isfinite(y).all():
            fails.append(f"{s}: {int((~np.isfinite(y)).sum())} non-finite elements")
            y = np.where(np.isfinite(y), y, 0.0)
        r, ye = ref[s], token_major(d, s, e_out[s]).astype(np.float64)
        ex = excess(y, r, _rms(e32[s].astype(np.float64) - r, 1)) / k_elem
        worst["elem"] = max(worst["elem"], float(ex.max()))
        if ex.max() > 1.0:
            i = np.unravel_index(int(np.argmax(ex)), ex.shape)
            fails.append(f"{s}: {int((ex > 1).sum())} of {ex.size} elements outside ulp16 / 2 + K_ELEM r(row); worst at [row, column] = "
                         f"{tuple(map(int, i))}: got {y[i]!r}, reference {r[i]!r}, ratio {ex.max():.3f}")
        sd, se = _stats(y - r), _stats(ye - r)
        for k, lim in l_stat.items():
            q = sd[k] / (lim * np.maximum(se[k], 1e-30))
            worst[k] = max(worst[k], float(q.max()))
            if q.max() > 1.0:
                fails.append(f"{s}: rms error over {k} [{int(np.argmax(q))}] is {q.max() * lim:.3f} x the emulation's (limit {lim})")
    if is_tail(d) and F(d, "GN"):
        worst["gn"] = gn_part_check(d, outs["OUT"], outs["GN_PART"])
        if not worst["gn"] <= 1.0:
            fails.append(f"GN_PART: not the sums of the returned output (error / tolerance {worst['gn']:.3f})")
    return fails, worst


def order_figures(d, ops, emu, ref, orders=ORDERS):
    """The emulation at the other accumulation orders against the one at 32: (largest excess, {statistic: largest relative difference})."""
    ex, spread = 0.0, dict.fromkeys(L_STAT, 0.0)
    for c in orders:
        o, _ = emulate(d, ops, chunk=c)
        for s in fp16_outputs(d):
            r = ref[s]
            y, y0 = (token_major(d, s, x[s]).astype(np.float64) for x in (o, emu[0]))
            ex = max(ex, float(excess(y, r, _rms(emu[1][s].astype(np.float64) - r, 1)).max()))
            s1, s0 = _stats(y - r), _stats(y0 - r)
            for k in spread:
                spread[k] = max(spread[k], float(np.abs(s1[k] / s0[k] - 1).max()))
    return ex, spread


def orders_of(name):
    """The other orders a sweep case is run at (the 264-workgroup cases at one)."""
    return (64,) if name.endswith("/wg264") else ORDERS


@functools.lru_cache(maxsize=None)
def figures(name):
    """order_figures of a sweep case, computed once per process."""
    d, _, ops, ref, emu = case(name)
    return order_figures(d, ops, emu, ref, orders=orders_of(name))


def measure_limits(names=None):
    """(largest excess, spreads) over the sweep: K_ELEM = 2 x, L_* = 1 + 3 x."""
    ex, spread = 0.0, dict.fromkeys(L_STAT, 0.0)
    for name in names or NAMES:
        e, s = figures(name)
        ex = max(ex, e)
        spread = {k: max(spread[k], s[k]) for k in spread}
    return ex, spread


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
KINDS = ("flat", "peaked", "equal_keys", "ln_offset", "wide_gates", "group_means")
PAD_VALUE = 60000.0


def pad_fill(d):
    """+-60000 alternating over the V^T pad columns and channels."""
    n = tv_of(d) - F(d, "T")
    return PAD_VALUE * np.where((np.arange(C)[:, None] + np.arange(n)[None, :]) % 2 == 0, 1.0, -1.0)[None]


def gn_stats_of(x, B, S, eps=1e-6):
    """(mean, 1 / (sigma + eps)) of every sample's 32 groups of 10 channels, from the fp16 bits of x [M][320] -> [B][32][2] float32."""
    g = np.asarray(x, np.float16).astype(np.float64).reshape(B, S, 32, 10)
    mu = g.mean(axis=(1, 3))
    sd = np.sqrt(((g - mu[:, None, :, None]) ** 2).mean(axis=(1, 3)))
    return np.stack([mu, 1.0 / (sd + eps)], axis=-1).astype(np.float32)


def make_logical(d, kind="flat", seed=0, pad=0.0):
    """The logical operands of descriptor d with the input shape `kind`.  Weights are N(0, 1 / K), biases N(0, 1/4)."""
    B, S = F(d, "B"), F(d, "S")
    M = B * S
    r = np.random.default_rng([seed, B, S, F(d, "T"), F(d, "MODE"), KINDS.index(kind)])
    w = lambda n, k: r.standard_normal((n, k)) / math.sqrt(k)
    if not is_tail(d):
        x = r.standard_normal((M, C))
        if kind == "group_means":      # a distinct mean and scale per group and per sample
            mu, sc = 3.0 * r.standard_normal((B, 1, 32, 1)), 0.25 + 2.0 * r.random((B, 1, 32, 1))
            x = (x.reshape(B, S, 32, 10) * sc + mu).reshape(M, C)
        x = x.astype(np.float16)
        return dict(X=x, GN_STATS=gn_stats_of(x, B, S), WC=w(C, C), WIN=w(3 * C, C), B_IN=0.5 * r.standard_normal(C))
    T, Tv = F(d, "T"), tv_of(d)
    L = dict(AO=r.standard_normal((M, C)), TOK=r.standard_normal((M, C)), X=r.standard_normal((M, C)), KC=r.standard_normal((B, T, C)),
             WSO=w(C, C), WQ=w(C, C), WCO=w(C, C), W1=w(8 * C, C), W2=w(C, 4 * C), WOUT=w(C, C), BSO=0.5 * r.standard_normal(C),
             BCO=0.5 * r.standard_normal(C), B1=0.5 * r.standard_normal(8 * C), B2=0.5 * r.standard_normal(C), BOUT=0.5 * r.standard_normal(C))
    vt = np.empty((B, C, Tv))
    vt[:, :, :T] = r.standard_normal((B, C, T))
    vt[:, :, T:] = np.broadcast_to(pad, (B, C, Tv - T))
    L["VT"] = vt
    if kind == "peaked":           # scores hundreds of log2 units apart: P subnormal or zero for most keys
        L["KC"] = L["KC"] * 16
    elif kind == "equal_keys":     # the output of the attention is the mean of V, to the accumulation and one rounding
        L["KC"] = np.broadcast_to(L["KC"][:, :1], L["KC"].shape).copy()
    elif kind == "ln_offset":      # a large common mean and a different one per column quarter
        L["TOK"] = L["TOK"] + 30.0 + np.repeat([-20.0, 0.0, 5.0, 40.0], 80)[None, :]
    elif kind == "wide_gates":     # gates spanning +-12: the exp2 argument overflows to inf on one side
        L["W1"][1::2] *= 4.0
        L["B1"][1::2] *= 4.0
    elif kind != "flat":
        raise ValueError(kind)
    return L


def make_inputs(d, kind="flat", seed=0, pad=0.0):
    return pack(d, make_logical(d, kind, seed, pad))


def sample_logical(d, L, b):
    """The logical operands of sample b alone (for a B = 1 descriptor of the same S and T)."""
    S = F(d, "S")
    out = {}
    for s, x in L.items():
        if s in ("AO", "TOK", "X"):
            out[s] = x[b * S:(b + 1) * S]
        elif s in ("KC", "VT"):
            out[s] = x[b:b + 1]
        elif s == "GN_STATS":
            out[s] = np.asarray(x).reshape(-1, 32, 2)[b:b + 1]
        else:
            out[s] = x
    return out


# ---- the descriptor sweep ------------------------------------------------------------------------------------------------------------
T_SWEEP = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 72, 73, 77, 79, 80)
PAD_T = (7, 9, 77)
PITCHED = dict(ld=(328, 336, 344, 352), ldk=328, ldvt=88, gap=24, krows=80, ldw=(328, 336, 344, 352, 1288, 328))
HEAD_PITCHED = dict(ld_x=344, ld_tok=336, ld_qk=656, gap=40, ldw=(328, 336))


def sweep():
    """[(name, descriptor, kind)] - the cases both tests/test_chain_ref_cpu.py (emulation) and tests/test_gpu_chain_ref.py (device) run."""
    out = [("tail/B1_S64", tail_desc(1, 64), "flat"),
           ("tail/B1_S64_gn", tail_desc(1, 64, gn=1), "flat"),
           ("tail/B3_S64_pitched", tail_desc(3, 64, **PITCHED), "flat"),
           ("tail/B2_S128_gn", tail_desc(2, 128, gn=1), "flat"),
           ("tail/B1_S192", tail_desc(1, 192), "flat")]
    out += [(f"tail/T{T}", tail_desc(1, 64, T=T, ldvt=88), "flat") for T in T_SWEEP]
    out += [(f"tail/{kind}", tail_desc(2, 128), kind) for kind in KINDS[1:5]]
    out += [("tail/wg264", tail_desc(4, 4224, gn=1), "flat")]
    out += [("head/B1_S64", head_desc(1, 64), "flat"),
            ("head/B3_S64_pitched", head_desc(3, 64, ld_vt=72, **HEAD_PITCHED), "group_means"),
            ("head/B2_S128", head_desc(2, 128), "flat"),
            ("head/group_means", head_desc(2, 128), "group_means"),
            ("head/B1_S192", head_desc(1, 192), "group_means"),
            ("head/wg264", head_desc(4, 4224), "group_means")]
    return out


SWEEP = sweep()
NAMES = [s[0] for s in SWEEP]
SEED = 7


@functools.lru_cache(maxsize=None)
def _case(name):
    _, d, kind = next(s for s in SWEEP if s[0] == name)
    ops = make_inputs(d, kind, seed=SEED)
    return d, kind, ops, reference(d, ops), emulate(d, ops)


def case(name):
    """(descriptor, kind, operands, reference, emulation) of a sweep case - computed once per process, shared, never modified."""
    return _case(name)
