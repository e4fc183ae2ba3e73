"""chain_ref's float64 reference and float32 emulation with the terms of the torch-norm kernels (attn_chain_kernel<KIND_HEAD_T> / <KIND_TAIL_T>,
run through tsd_debug_chain_run_affine): gamma / beta on the head's GroupNorm and on the three LayerNorms, rstd = 1 / sqrt(var + eps) and
the exact GELU.  chain_ref writes its norms and its GELU inline, so both functions are restated here formula for formula (a CPU test holds them
to chain_ref's, exactly, at the identity affine with the reference's rstd and the tanh GELU).  Operands, descriptors, layout and `check` are chain_ref's.

aff = (gn_w, gn_b, ln0_w, ln0_b, ln1_w, ln1_b, ln2_w, ln2_b), TSD_CA_* order; gamma ~ U(0.5, 1.5), beta ~ U(-0.5, 0.5).  |gamma| <= 1.5 scales
a normalised value, and the error of the fp16 rounding behind it, by at most 1.5 - the emulation carries the same factor, so chain_ref's
limits, which are ratios to the emulation's own error, hold as they stand: K_ELEM = 10.4, L_STAT whole 1.017, rows 2.0, cols 2.0, tiles 1.36.
No limit was widened and no element is excluded."""
import ctypes as C
import math

import numpy as np

import chain_ref as R
import replay

f32 = np.float32
CA_COUNT, REF_RSTD = 8, 1       # TSD_CA_COUNT, TSD_CAF_REF_RSTD
IDENTITY = tuple(np.ones(R.C) if i % 2 == 0 else np.zeros(R.C) for i in range(CA_COUNT))
_erf = np.vectorize(math.erf, otypes=[np.float64])


def draw_affine(seed):
    r = np.random.default_rng([seed, 320])
    return tuple((r.uniform(0.5, 1.5, R.C) if i % 2 == 0 else r.uniform(-0.5, 0.5, R.C)).astype(f32) for i in range(CA_COUNT))


def _ln64(x, eps, w, b, torch):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / (np.sqrt(var + eps) if torch else np.sqrt(var) + eps) * w + b


def _ln32(v, eps, w, b, torch):
    mu = v.mean(axis=1, keepdims=True, dtype=f32)
    var = ((v - mu) ** 2).mean(axis=1, keepdims=True, dtype=f32)
    rs = f32(1) / np.sqrt(var + f32(eps)) if torch else f32(1) / (np.sqrt(var) + f32(eps))
    return R._h(((v - mu) * rs) * f32(w) + f32(b))


def _gelu_erf32(x):
    """The device's evaluation (gelu_erf_f, csrc/common.h): Abramowitz-Stegun 7.1.26 in float32."""
    z = np.abs(x) * f32(0.7071067811865476)
    t = f32(1) / (f32(1) + f32(0.3275911) * z)
    poly = t * (f32(0.254829592) + t * (f32(-0.284496736) + t * (f32(1.421413741) + t * (f32(-1.453152027) + t * f32(1.061405429)))))
    return f32(0.5) * x * (f32(1) + np.copysign(f32(1) - poly * np.exp2(f32(-R.LOG2E) * z * z).astype(f32), x))


def _gelu64(x, erf):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0))) if erf else R._gelu_tanh(x)


def _inputs(d, ops, dt):
    L = {k: v.astype(dt) for k, v in R.unpack(d, {s: ops[s] for s in ops if s not in R.OUTPUTS}).items()}
    B, S = R.F(d, "B"), R.F(d, "S")
    if R.is_tail(d):
        return L, B, S, dt(R.bits_f32(R.F(d, "EPS")))
    st = L["GN_STATS"].reshape(B, 32, 2)
    mean, rstd = (np.repeat(np.repeat(st[:, :, i], 10, axis=1), S, axis=0) for i in (0, 1))
    return L, mean, rstd, dt(R.bits_f32(R.F(d, "EPS")))


def reference(d, ops, aff=IDENTITY, erf=True, torch=True):
    """chain_ref.reference, formula for formula, with the affine terms, the selected rstd and the selected GELU."""
    if not R.is_tail(d):
        L, mean, rstd, eps = _inputs(d, ops, np.float64)
        tok = ((L["X"] - mean) * rstd * aff[0] + aff[1]) @ L["WC"].T + L["B_IN"]
        qkv = _ln64(tok, eps, aff[2], aff[3], torch) @ L["WIN"].T
        return {"HTOK": tok, "QK": qkv[:, :2 * R.C], "HVT": qkv[:, 2 * R.C:]}
    L, B, S, eps = _inputs(d, ops, np.float64)
    T, scale = R.F(d, "T"), float(R.bits_f32(R.F(d, "SCALE")))
    tok2 = L["AO"] @ L["WSO"].T + L["BSO"] + L["TOK"]
    q = _ln64(tok2, eps, aff[4], aff[5], torch) @ L["WQ"].T
    attn = np.empty_like(q)
    for b in range(B):
        k, v = L["KC"][b], L["VT"][b][:, :T].T
        for h in range(R.HEADS):
            c = slice(h * R.HD, (h + 1) * R.HD)
            s = scale * (q[b * S:(b + 1) * S, c] @ k[:, c].T)
            w = np.exp(s - s.max(axis=1, keepdims=True))
            attn[b * S:(b + 1) * S, c] = (w / w.sum(axis=1, keepdims=True)) @ v[:, c]
    tok3 = tok2 + attn @ L["WCO"].T + L["BCO"]
    h1 = _ln64(tok3, eps, aff[6], aff[7], torch) @ L["W1"].T + L["B1"]
    tok4 = tok3 + (h1[:, 0::2] * _gelu64(h1[:, 1::2], erf)) @ L["W2"].T + L["B2"]
    return {"OUT": L["X"] + tok4 @ L["WOUT"].T + L["BOUT"]}


def emulate(d, ops, aff=IDENTITY, erf=True, torch=True, chunk=32):
    """chain_ref.emulate (no mutation), rounding point for rounding point, with the same three choices."""
    h, mm = R._h, R._mm
    if not R.is_tail(d):
        L, mean, rstd, eps = _inputs(d, ops, f32)
        tok32 = mm(h((L["X"] - mean) * (rstd * f32(aff[0])) + f32(aff[1])), L["WC"], chunk) + L["B_IN"]
        a = _ln32(tok32, eps, aff[2], aff[3], torch)
        y32 = {"HTOK": tok32, "QK": mm(a, L["WIN"][:2 * R.C], chunk), "HVT": mm(a, L["WIN"][2 * R.C:], chunk)}
        vt = h(y32["HVT"]).reshape(R.F(d, "B"), R.F(d, "S"), R.C).transpose(0, 2, 1)
        return R.pack(d, {"HTOK": h(tok32), "QK": h(y32["QK"]), "HVT": vt}), y32
    L, B, S, eps = _inputs(d, ops, f32)
    T, Tv = R.F(d, "T"), R.tv_of(d)
    qscale = f32(f32(R.bits_f32(R.F(d, "SCALE"))) * f32(R.LOG2E))
    res = L["TOK"] + (mm(L["AO"], L["WSO"], chunk) + L["BSO"])
    qa = h(mm(_ln32(res, eps, aff[4], aff[5], torch), L["WQ"], chunk) * qscale)
    valid = np.arange(80) < T
    attn = np.empty((B * S, R.C), f32)
    for b in range(B):
        kp, vp = np.zeros((80, R.C), f32), np.zeros((80, R.C), f32)
        kp[:T] = L["KC"][b]
        vp[:Tv] = L["VT"][b].T
        for hd in range(R.HEADS):
            c = slice(hd * R.HD, (hd + 1) * R.HD)
            s = np.where(valid[None, :], qa[b * S:(b + 1) * S, c] @ kp[:, c].T, f32(-1.0e30))
            p = np.where(valid[None, :], h(np.exp2(s - s.max(axis=1, keepdims=True))), f32(0))
            attn[b * S:(b + 1) * S, c] = h((p @ vp[:, c]) * (f32(1) / p.sum(axis=1, dtype=f32))[:, None])
    res = res + (mm(attn, L["WCO"], chunk) + L["BCO"])
    a = _ln32(res, eps, aff[6], aff[7], torch)
    ha, hg = mm(a, L["W1"][0::2], chunk) + L["B1"][0::2], mm(a, L["W1"][1::2], chunk) + L["B1"][1::2]
    res = res + (mm(h(ha * (_gelu_erf32(hg) if erf else R._gelu32(hg))), L["W2"], chunk) + L["B2"])
    y32 = L["X"] + (mm(h(res), L["WOUT"], chunk) + L["BOUT"])
    outs = R.pack(d, {"OUT": h(y32)})
    if R.F(d, "GN"):
        f = h(y32).reshape(B, S // 32, 32, 32, 10)
        outs["GN_PART"] = np.ascontiguousarray(np.stack([f.sum(axis=(2, 4), dtype=f32), (f * f).sum(axis=(2, 4), dtype=f32)], axis=-1).ravel())
    return outs, {"OUT": y32}


def run(ctx, d, ops, aff, flags=0):
    """tsd_debug_chain_run_affine through replay.run (which holds the extents to chain_ref's): (status, outputs, info {CHANGED, RAN})."""
    L = replay.lib()
    vecs = [np.ascontiguousarray(v, f32) for v in aff]
    ptrs = (C.c_void_p * CA_COUNT)(*[v.ctypes.data for v in vecs])
    L.chain_run_affine_bound = lambda c, dd, n, i, o, e, info: L.tsd_debug_chain_run_affine(c, dd, n, i, o, e, info, R.CI["COUNT"], ptrs, flags)
    rc, outs, info = replay.run("chain_run_affine_bound", ctx, d, ops, R.CO, R.INPUTS, R.OUTPUTS, R.dtype_of, R.extents)
    return rc, outs, {k: int(info[v]) for k, v in R.CI.items() if k != "COUNT"}
