"""tests/gemm_ref.py on the CPU: the fp64 reference is pinned against the oracle and torch for the conv / dense operand modes, the
bound accepts legitimately rounded results (fp32 accumulation in several blocked K orders, then the fp16 store) and rejects each
of the faults it is there to catch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
import replay
from oracle import ops as oops

E = G.EPI


def _nchw(d, flat, slot, C):
    """Device NHWC source (pitch lda) -> float64 [B][C][Hs][Ws]."""
    g = lambda k: int(d[G.GD[k]])  # noqa: E731
    ld = g({"A0": "LDA0", "A1": "LDA1", "A2": "LDA2"}[slot])
    px = G.samples(d) * g("HS") * g("WS")
    x = np.concatenate([flat.astype(np.float64), np.zeros(px * ld - flat.size)]).reshape(G.samples(d), g("HS"), g("WS"), ld)
    return torch.from_numpy(np.ascontiguousarray(x[..., :C].transpose(0, 3, 1, 2)))


def _torch_conv(d, ops, pad_br):
    g = lambda k: int(d[G.GD[k]])  # noqa: E731
    N, Cin = g("N"), g("CIN")
    x = _nchw(d, ops["A0"], "A0", Cin)
    if g("UPS"):
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    w = torch.from_numpy(ops["W"].astype(np.float64)[np.arange(N)[:, None] * g("LDW") + np.arange(9 * Cin)[None, :]])
    w = w.reshape(N, 3, 3, Cin).permute(0, 3, 1, 2)
    p = g("PAD")
    y = F.conv2d(F.pad(x, (p, pad_br, p, pad_br)), w, stride=g("STRIDE"))
    c1, c2 = g("CIN1"), g("CIN2")
    if c1:
        s = _nchw(d, ops["A1"], "A1", c1)
        if c2:
            s = torch.cat([s, _nchw(d, ops["A2"], "A2", c2)], dim=1)
        w1 = torch.from_numpy(G.weight(d, ops)[:, 9 * Cin:]).reshape(N, c1 + c2, 1, 1)
        y = y + F.conv2d(s, w1)
    return y.permute(0, 2, 3, 1).reshape(-1, N).numpy()  # [B*Ho*Wo][N]


CONV_CASES = {
    "stride2_odd": dict(B=2, Hs=9, Ws=7, Cin=64, N=20, stride=2),
    "stride2_even": dict(B=1, Hs=8, Ws=10, Cin=64, N=12, stride=2),
    "upsample": dict(B=2, Hs=3, Ws=5, Cin=64, N=8, ups=1),
    "pad0": dict(B=1, Hs=6, Ws=5, Cin=64, N=8, pad=0),
    "pad_0_1_stride2": dict(B=2, Hs=8, Ws=6, Cin=64, N=8, stride=2, pad=0, pad_br=1),
    "pitched_input": dict(B=1, Hs=4, Ws=4, Cin=64, N=8, lda0=80),
    "skip_concat": dict(B=2, Hs=5, Ws=3, Cin=64, N=8, Cin1=64, Cin2=128, lda1=72, lda2=136),
    "one_pixel": dict(B=3, Hs=1, Ws=1, Cin=64, N=4),
}


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_reference_matches_torch_float64(name):
    c = dict(CONV_CASES[name])
    pad_br = c.get("pad_br", c.get("pad", 1))
    d = G.conv_desc(**c)
    ops = G.make_operands(d, 7)
    M = int(d[G.GD["M"]])
    ref, _, _ = G.reference(d, ops, np.arange(M))
    np.testing.assert_allclose(ref, _torch_conv(d, ops, pad_br), rtol=1e-12, atol=1e-12)


def test_conv_reference_matches_the_oracle_conv2d():
    """The W layout k_pack_conv writes ([N][tap][Cin], tap = kh * 3 + kw) against oracle.ops.conv2d's OIHW cross-correlation,
    with the encoder's (0, 1) padding."""
    d = G.conv_desc(B=1, Hs=7, Ws=6, Cin=64, N=8, stride=2, pad=0, pad_br=1)
    ops = G.make_operands(d, 11)
    g = lambda k: int(d[G.GD[k]])  # noqa: E731
    x = _nchw(d, ops["A0"], "A0", 64).numpy()[0]
    w = ops["W"].astype(np.float64).reshape(8, 3, 3, 64).transpose(0, 3, 1, 2)
    y = oops.conv2d(x, w, None, stride=(2, 2), pad_hw=((0, 1), (0, 1)))
    ref, _, _ = G.reference(d, ops, np.arange(g("M")))
    np.testing.assert_allclose(ref, y.transpose(1, 2, 0).reshape(-1, 8), rtol=1e-12, atol=1e-12)


def test_dense_reference_matches_oracle_linear_with_concat_and_batch_strides():
    d = G.dense_desc(M=37, N=24, K=192, K0=64, lda0=72, lda1=136, ldw=200, ldc=28, batch=3, sa=37 * 136 + 5, sw=24 * 200 + 8,
                     sc=37 * 28 + 4)
    ops = G.make_operands(d, 5)
    ref, _, _ = G.reference(d, ops, np.arange(3 * 37))
    for b in range(3):
        a0 = ops["A0"].astype(np.float64)[b * int(d[G.GD["SA"]]) + np.arange(37)[:, None] * 72 + np.arange(64)[None, :]]
        a1 = ops["A1"].astype(np.float64)[b * int(d[G.GD["SA"]]) + np.arange(37)[:, None] * 136 + np.arange(128)[None, :]]
        w = ops["W"].astype(np.float64)[b * int(d[G.GD["SW"]]) + np.arange(24)[:, None] * 200 + np.arange(192)[None, :]]
        np.testing.assert_allclose(ref[b * 37:(b + 1) * 37], oops.linear(np.concatenate([a0, a1], 1), w), rtol=1e-12, atol=1e-12)


def test_extents_and_gaps():
    """Pitch gaps are NaN in the generated operands and never read by the reference."""
    d = G.dense_desc(M=5, N=8, K=64, lda0=70, ldw=66)
    ops = G.make_operands(d, 1)
    e = G.extents(d)
    assert e["A0"] == 4 * 70 + 64 and e["W"] == 7 * 66 + 64 and e["C"] == 4 * 8 + 8
    assert np.isnan(ops["A0"][64:70]).all() and np.isfinite(ops["A0"][:64]).all()
    ref, _, _ = G.reference(d, ops, np.arange(5))
    assert np.isfinite(ref).all()


# ---- a host model of the kernel: fp32 accumulation over 64-deep K tiles in a chosen order, fp32 epilogue, fp16 store ----------
def _simulate(d, ops, order="forward", drop=None, bias_shift=None, res_shift=None, tap_fault=None):
    g = lambda k: int(d[G.GD[k]])  # noqa: E731
    M, N, K, epi, B = g("M"), g("N"), g("K"), g("EPI"), g("BATCH")
    rows = np.arange(M * B)
    bz, m = rows // M, rows % M
    A = G.gather_a(d, ops, rows)
    if tap_fault is not None:  # row r's tap t reads the wrapped pixel (padding handled wrong) instead of zero
        r, t, src = tap_fault
        Cin = g("CIN")
        A[r, t * Cin:(t + 1) * Cin] = G.gather_a(d, ops, [src])[0, 4 * Cin:5 * Cin]
    acc = np.zeros((M * B, N), np.float32)
    nt = K // 64
    tiles = {"forward": range(nt), "reverse": range(nt - 1, -1, -1)}.get(order)
    for b in range(B):
        sel = bz == b
        Wm = G.weight(d, ops, b).astype(np.float32)
        Ab = A[sel].astype(np.float32)
        if order == "split2":  # two K halves summed separately, then added (the split-K hand-off)
            h = nt // 2
            parts = [np.zeros((sel.sum(), N), np.float32) for _ in range(2)]
            for t in range(nt):
                p = parts[0 if t < h else 1]
                p += Ab[:, t * 64:(t + 1) * 64] @ Wm[:, t * 64:(t + 1) * 64].T
            acc[sel] = parts[0] + parts[1]
            continue
        a = np.zeros((sel.sum(), N), np.float32)
        for t in tiles:
            part = Ab[:, t * 64:(t + 1) * 64] @ Wm[:, t * 64:(t + 1) * 64].T
            if drop is not None and drop[1] == t:
                part[(np.flatnonzero(sel) >= drop[0]) & (np.flatnonzero(sel) < drop[0] + 64)] = 0
            a += part
        acc[sel] = a
    v = acc * np.float32(G.out_scale(d))
    if epi & E["BIAS_M"]:
        v += ops["BIAS"][m][:, None]
    if epi & E["BIAS_N"]:
        bias = ops["BIAS"][:N].copy()
        if bias_shift is not None:
            bias[bias_shift] = ops["BIAS"][bias_shift + 1]
        v += bias[None, :]
    if epi & E["ROWVEC"]:
        v += ops["ROWVEC"][(m // g("ROWS_PER_BATCH"))[:, None] * g("ROWVEC_LD") + np.arange(N)[None, :]]
    if epi & E["RESIDUAL"]:
        rr = m.copy()
        if epi & E["RES_UPS"]:
            Ho, Wo = g("HO"), g("WO")
            oy, ox = (m % (Ho * Wo)) // Wo, m % Wo
            rr = ((m // (Ho * Wo)) * (Ho // 2) + oy // 2) * (Wo // 2) + ox // 2
        if res_shift is not None:
            rr[res_shift] += 1
        v += ops["R"][(bz * g("SR") + rr * g("LDR"))[:, None] + np.arange(N)[None, :]].astype(np.float32)
    if epi & E["GEGLU"]:
        a, gt = v[:, 0::2], v[:, 1::2]
        v = (a * (gt * (np.float32(1) / (np.float32(1) + np.exp2(np.float32(-2 * 0.7978845608028654 * 1.4426950408889634) *
                                                                    (gt + np.float32(0.044715) * gt * gt * gt)))))).astype(np.float32)
    cols = G.c_cols(d)
    out_dt = np.float32 if epi & E["OUT_F32"] else np.float16
    C = np.full(G.extents(d)["C"], G.NAN32 if out_dt == np.float32 else G.NAN16, out_dt)
    idx = (bz * g("SC") + m * g("LDC"))[:, None] + np.arange(cols)[None, :]
    C[idx] = v[:, :cols].astype(out_dt)
    return C


def _check(d, ops, C, rows=None):
    g = lambda k: int(d[G.GD[k]])  # noqa: E731
    rows = np.arange(g("M") * g("BATCH")) if rows is None else rows
    return G.check(d, ops, {"C": C}, rows)


PROD = E["BIAS_N"] | E["RESIDUAL"]


@pytest.mark.parametrize("order", ["forward", "reverse", "split2"])
@pytest.mark.parametrize("case", ["conv_res", "dense_geglu", "dense_f32_scaled", "conv_rowvec_ups_res"])
def test_bound_accepts_rounded_results(case, order):
    if case == "conv_res":
        d = G.conv_desc(B=2, Hs=6, Ws=5, Cin=128, N=40, epi=PROD)
    elif case == "dense_geglu":
        d = G.dense_desc(M=96, N=48, K=640, epi=E["BIAS_N"] | E["GEGLU"])
    elif case == "dense_f32_scaled":
        d = G.dense_desc(M=70, N=24, K=256, epi=E["BIAS_N"] | E["OUT_F32"], out_scale=0.125)
    else:
        d = G.conv_desc(B=2, Hs=4, Ws=6, Cin=64, N=16, ups=1, epi=E["BIAS_N"] | E["ROWVEC"] | E["RESIDUAL"] | E["RES_UPS"],
                        rowvec_ld=16, rows_per_batch=8 * 12)
    ops = G.make_operands(d, 3, scale={"W": 1.7 / np.sqrt(int(d[G.GD["K"]])) * (8.0 if case == "dense_f32_scaled" else 1.0)})
    assert _check(d, ops, _simulate(d, ops, order)) == []


def _residual_desc():
    return G.conv_desc(B=3, Hs=5, Ws=5, Cin=128, N=16, epi=PROD)


def test_rejects_one_k_tile_dropped_for_one_tile_row():
    d = G.dense_desc(M=192, N=32, K=640, epi=E["BIAS_N"])
    ops = G.make_operands(d, 4)
    assert _check(d, ops, _simulate(d, ops, drop=(64, 9)))


def test_rejects_residual_one_row_off_at_a_sample_boundary():
    d = _residual_desc()
    ops = G.make_operands(d, 4)
    assert _check(d, ops, _simulate(d, ops, res_shift=24))  # last row of sample 0 reads sample 1's first
    assert _check(d, ops, _simulate(d, ops, res_shift=24), rows=G.sample_rows(d, 0, n_random=0))


def test_rejects_bias_on_the_wrong_column():
    d = G.dense_desc(M=64, N=40, K=128, epi=E["BIAS_N"])
    ops = G.make_operands(d, 4)
    assert _check(d, ops, _simulate(d, ops, bias_shift=37))


def test_rejects_one_border_tap_padded_wrong():
    d = G.conv_desc(B=1, Hs=6, Ws=6, Cin=64, N=8)
    ops = G.make_operands(d, 4)
    # output pixel (0, 3), tap (kh 0, kw 1) lies above the image: it must read zeros, the fault reads pixel (5, 3) (wrap-around)
    bad = _simulate(d, ops, tap_fault=(3, 1, 5 * 6 + 3))
    assert _check(d, ops, bad)
    assert _check(d, ops, bad, rows=G.sample_rows(d, 0, n_random=0))


def test_rejects_two_geglu_pairs_swapped():
    d = G.dense_desc(M=64, N=32, K=128, epi=E["BIAS_N"] | E["GEGLU"])
    ops = G.make_operands(d, 4)
    C = _simulate(d, ops)
    ldc = int(d[G.GD["LDC"]])
    C[5 * ldc + 2], C[5 * ldc + 3] = C[5 * ldc + 3], C[5 * ldc + 2]
    assert _check(d, ops, C)


def test_rejects_an_element_left_as_the_nan_pattern():
    d = G.dense_desc(M=64, N=16, K=64, ldc=24)
    ops = G.make_operands(d, 4)
    C = _simulate(d, ops)
    C[63 * 24 + 15] = G.NAN16
    assert _check(d, ops, C)


def _gn_desc():
    return G.conv_desc(B=3, Hs=8, Ws=8, Cin=64, N=40, epi=E["BIAS_N"] | E["GNSTATS"], gn_groups=4, gn_rps=64, gn_nslab=2)


def _gn_partials(d, C, dt=np.float32):
    ref, _, _ = G.gn_reference(d, C)
    return ref.astype(dt)


def test_gn_statistics_accepts_fp32_sums_and_rejects_a_swapped_slab():
    d = _gn_desc()
    ops = G.make_operands(d, 4)
    C = _simulate(d, ops)
    gn = _gn_partials(d, C)
    assert G.check_gn(d, C, gn) == []
    G_, ns = 4, 2
    swapped = gn.reshape(3, ns, G_, 2).copy()
    swapped[1, [0, 1]] = swapped[1, [1, 0]]  # sample 1: slab 0 written into slab 1's slot and back
    assert G.check_gn(d, C, swapped.ravel())


def test_descriptor_enum_parsed_from_the_header():
    assert G.GD["VERSION"] == 0 and G.COUNT == max(v for k, v in G.GD.items() if k != "COUNT") + 1
    assert set(G.INPUTS + G.OUTPUTS) == {k for k in G.GO if k != "COUNT"}
    assert G.EPI == {"BIAS_N": 1, "BIAS_M": 2, "ROWVEC": 4, "RESIDUAL": 8, "RES_UPS": 16, "GEGLU": 32, "OUT_F32": 64, "GNSTATS": 128}


def test_replay_entry_sizes_like_the_reference_and_refuses_inconsistent_geometry():
    """tsd_debug_gemm_run with no operands only sizes (no device needed).  Its extents equal gemm_ref's; a conv descriptor whose
    output size does not follow from source, stride and padding - or whose first-tap coordinate would not fit the kernel's
    11-bit field - is refused before anything is allocated."""
    from tsd._lib import lib

    def size(d):
        return replay.size("tsd_debug_gemm_run", d, extra=(-1,))

    assert lib().tsd_debug_gemm_run(None, None, 0, -1, None, None, None, None) != 0
    good = [G.conv_desc(B=2, Hs=9, Ws=7, Cin=64, N=20, stride=2, epi=PROD), G.conv_desc(B=1, Hs=8, Ws=6, Cin=64, N=8, stride=2, pad=0, pad_br=1),
            G.conv_desc(B=2, Hs=5, Ws=3, Cin=64, N=8, Cin1=64, Cin2=128, epi=E["BIAS_N"] | E["GNSTATS"], gn_groups=4, gn_rps=15, gn_nslab=0),
            G.dense_desc(M=37, N=24, K=192, K0=64, batch=3, sa=37 * 128 + 64, sw=24 * 192, sc=37 * 24, epi=E["BIAS_N"] | E["GEGLU"])]
    for d in good[:2] + good[3:]:
        rc, ext = size(d)
        assert rc == 0 and {s: int(ext[G.GO[s]]) for s in G.extents(d)} == G.extents(d)
    bad_wo = G.conv_desc(B=1, Hs=8, Ws=8, Cin=64, N=8, stride=2)
    bad_wo[G.GD["WO"]] += 1                                              # output wider than the source allows
    wide = G.conv_desc(B=2, Hs=4, Ws=1500, Cin=64, N=8, stride=2, ups=1)  # first tap column beyond 11 bits
    for d in (bad_wo, wide, good[2]):                                     # (gn_nslab 0 cannot be sized)
        assert size(d)[0] == -1
