"""No GPU: tests/elem_ref.py - the fp64 references, the derived bounds, the expected bits of the movement kernels and the numpy
emulation of csrc/kernels_elementwise.hip - is itself tested.  Its operand extents agree with tsd_debug_elem_run's sizing-only mode;
the references agree with the oracle's own ops; the emulation of the device arithmetic stays inside every bound; every seeded defect is
rejected on a sweep case the GPU test runs as well; the SMALL_LINEAR bound stays under its cap; no time-embedding frequency sits at a
float32 rounding midpoint."""
import numpy as np
import pytest

import elem_ref as E
import replay
from oracle import ops as O

SWEEP = E.sweep()
BY_NAME = {s[0]: s for s in SWEEP}
SEED = 11


def _size(d, n=None):
    info = np.full(E.EI["COUNT"], -1, np.int64)
    rc, ext = replay.size("tsd_debug_elem_run", d, n, info)
    return rc, {s: int(ext[E.EO[s]]) for s in E.INPUTS + E.OUTPUTS}, info


def _case(name):
    _, d, kind, _ = BY_NAME[name]
    return d, E.make_inputs(d, SEED, kind)


# ---- extents against the entry's sizing-only mode ------------------------------------------------------------------------------------
def test_sweep_covers_every_mode_and_names_are_unique(tsd_mod):
    assert len(BY_NAME) == len(SWEEP)
    assert {E.mode_of(d) for _, d, _, _ in SWEEP} == set(E.MODES)


def test_extents_agree_with_the_entry(tsd_mod):
    for name, d in [(s[0], s[1]) for s in SWEEP] + E.refusals():
        rc, ext, info = _size(d)
        assert rc == 0, (name, replay.lib().tsd_last_error().decode())
        assert ext == E.extents(d), f"{name}: the entry and tests/elem_ref.py size the operands differently"
        assert (info[:E.EI["COUNT"]] == 0).all()


def test_unsizable_descriptors_are_refused(tsd_mod):
    good = E.small_linear(3, 136, 17)
    assert _size(good)[0] == 0
    assert _size(good, n=E.COUNT - 1)[0] != 0
    for field, v in (("VERSION", 2), ("MODE", E.EM["COUNT"]), ("MODE", -1), ("B", 0), ("K", 0), ("N", 0), ("LDX", 128), ("LDW", 135), ("LDY", 16),
                     ("SILU", 2), ("HAS_BIAS", -1), ("N", 1 << 40), ("B", 65)):
        d = good.copy()
        d[E.ED[field]] = v
        assert _size(d)[0] != 0, field
    for d in (E.time_embedding(0, 1.0), E.geglu(0, 8), E.quick_gelu(0), E.unary(3, 16), E.clip_embed(1, 0, 11, 8), E.clip_embed(1, 5, 0, 8),
              E.chw_to_nhwc(1, 4, 2, 2, 5, 8), E.chw_to_nhwc(1, 4, 0, 2, 4, 8), E.im2col(1, 0, 2, 2), E.nhwc_to_chw(1, 1, 5, 2, 2, 4),
              E.nhwc_to_chw(2, 1, 5, 2, 2, 8), E.f32_to_f16_rows(3, 5, 4, 4), E.f32_to_f16_rows(3, 5, 8, 2), E.f16_to_f32_rows(3, 5, 4),
              E.transpose_to_f16(1, 5, 3, 4, 4), E.transpose_to_f16(1, 5, 3, 8, 2), E.pack_conv(3, 5, 3, 2, 8), E.pack_conv(3, 5, 3, 4, 4),
              E.pack_conv(3, 5, 0, 4, 8), E.pack_linear(6, 5, 4), E.pack_linear(5, 5, 8, 1), E.pack_bias(6, 4), E.pack_bias(5, 8, 1),
              E.pack_im2col_w(3, 8, 0), E.encoder_sample(2, 6, 7), E.encoder_sample(0, 6, 8)):
        assert _size(d)[0] != 0, (E.mode_of(d), d)


# ---- the references against the oracle's own ops, in float64 -------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", ["sl_b5_k320_n48_silu0", "sl_b5_k320_n48_silu1", "sl_pitches_silu1", "sl_no_bias", "sl_k2560_b3_n17_silu1"])
def test_small_linear_reference_agrees_with_the_oracle(name):
    d, ops = _case(name)
    x, w, b = E.sl_operands(d, ops)
    want = O.linear(O.silu(x) if E.F(d, "SILU") else x, w, b if "BIAS" in ops else None)
    assert _rel(E.reference(d, ops)[0], want) <= 1e-12


def test_activation_references_agree_with_the_oracle():
    for name, fn in (("unary_silu_grid", O.silu), ("unary_gelu_grid", O.gelu_tanh), ("quick_gelu_all_f16", O.quick_gelu)):
        d, ops = _case(name)
        x = ops["X"].astype(np.float64)
        ok = np.abs(x) < 700           # the oracle's exp overflows beyond
        with np.errstate(over="ignore"):
            assert _rel(E.reference(d, ops)[0][ok], fn(x[ok])) <= 1e-12, name
    d, ops = _case("unary_pixel")
    x = ops["X"].astype(np.float64)
    ok = np.isfinite(x)
    assert _rel(E.reference(d, ops)[0][ok], O.rescale_to_u8_range(x[ok])) <= 1e-12
    d, ops = _case("geglu_random")
    v = ops["X"].astype(np.float64).reshape(3, 20, 2)
    assert _rel(E.reference(d, ops)[0], v[..., 0] * O.gelu_erf(v[..., 1])) <= 2.0 ** -23   # the oracle returns its erf-GELU as float32


def test_time_embedding_reference_agrees_with_the_oracle():
    """The oracle rounds f and f t to float32 as the kernel does and takes cos / sin in float32: one float32 rounding of the reference,
    to the last place or the one beside it."""
    for t in (0.0, 1.0, 20.0, 980.0, 999.0, 333.25):
        d = E.time_embedding(1, t)
        ref, bd = E.reference(d, {})
        want = O.time_embedding(t).astype(np.float64)
        assert np.abs(ref[0] - want).max() <= 2.0 ** -23
        assert (bd <= 2.0 ** -24 * 1.000002).all()


def test_time_embedding_frequencies_are_no_rounding_midpoints():
    f64, f32 = E.time_freqs()
    other = np.where(f64 >= f32, np.nextafter(f32, np.float32(np.inf)), np.nextafter(f32, np.float32(-np.inf))).astype(np.float64)
    mid = (f32.astype(np.float64) + other) / 2
    assert (np.abs(f64 - mid) / f64 > 2.0 ** -40).all()
    assert f32[0] == 1.0 and abs(float(f32[159]) - 1e-4 * 10000 ** (1 / 160)) < 1e-10


def test_layouts_agree_with_the_oracle_convolution():
    """im2col(x) . pack_im2col_w(pack_conv(w))^T is the oracle's 3x3 convolution: the three layouts as one statement, on fp16-exact
    values (every product and sum is exact in float64)."""
    r = np.random.default_rng(5)
    for C in (3, 4, 7):
        B, H, W, Ocount = 2, 5, 3, 3
        x = (r.integers(-64, 64, (B, C, H, W)) / 16).astype(np.float32)
        w = (r.integers(-64, 64, (Ocount, C, 3, 3)) / 16).astype(np.float32)
        d = E.im2col(B, C, H, W)
        A = E.expected(d, {"X": x.ravel()}).astype(np.float64).reshape(B, H * W, 64)
        dp = E.pack_conv(Ocount, C, 3, 4, 8)
        packed = E.expected(dp, {"X": w.ravel()})
        dw = E.pack_im2col_w(4, 8, C)
        Wm = E.expected(dw, {"X": packed}).astype(np.float64).reshape(4, 64)
        for b in range(B):
            want = O.conv2d(x[b].astype(np.float64), w.astype(np.float64), padding=(1, 1))
            got = (A[b] @ Wm.T).T.reshape(4, H, W)
            assert _rel(got[:Ocount], want) <= 1e-12 and (got[Ocount:] == 0).all()
        # the NHWC conversion holds the same pixels, channel-minor
        dn = E.chw_to_nhwc(B, C, H, W, C, 8)
        y = E.expected(dn, {"X": x.ravel()}).reshape(B, H * W, 8)
        assert np.array_equal(y[:, :, :C].astype(np.float32), x.reshape(B, C, H * W).transpose(0, 2, 1)) and (y[:, :, C:] == 0).all()
        back = E.expected(E.nhwc_to_chw(1, B, C, H, W, 8), {"X": y.ravel()[:(B * H * W - 1) * 8 + C]})
        assert np.array_equal(back, x.ravel())


def test_linear_layouts_agree_with_the_oracle_and_chunk_order():
    r = np.random.default_rng(6)
    N, K = 6, 5
    w = (r.integers(-64, 64, (N, K)) / 16).astype(np.float32)
    b = (r.integers(-64, 64, N) / 16).astype(np.float32)
    x = (r.integers(-64, 64, (4, K)) / 16).astype(np.float64)
    want = O.linear(x, w.astype(np.float64), b.astype(np.float64))
    for il in (0, 1):
        pw = E.expected(E.pack_linear(N, K, 8, il), {"X": w.ravel()}).astype(np.float64).reshape(N, 8)
        pb = E.expected(E.pack_bias(N, 8, il), {"X": b}).astype(np.float64)
        assert (pw[:, K:] == 0).all() and (pb[N:] == 0).all()
        got = x @ pw[:, :K].T + pb[:N]
        if il:   # chunk(2): the first half of the features is `a`, the second the gate; packed as (a, gate) pairs
            a, g = want[:, :N // 2], want[:, N // 2:]
            assert _rel(got[:, 0::2], a) <= 1e-12 and _rel(got[:, 1::2], g) <= 1e-12
            dg = E.geglu(4, N // 2)
            ref, _ = E.reference(dg, {"X": got.astype(np.float16).ravel()})
            h = got.astype(np.float16).astype(np.float64)
            assert _rel(ref, h[:, 0::2] * O.gelu_erf(h[:, 1::2])) <= 2.0 ** -23   # the oracle returns its erf-GELU as float32
        else:
            assert _rel(got, want) <= 1e-12
    # the transpose is the K-major W operand of matmul: a @ b == a @ transpose(b)^T
    bm = (r.integers(-64, 64, (2, K, 3)) / 16).astype(np.float32)
    t = E.expected(E.transpose_to_f16(2, K, 3, 8, 4), {"X": bm.ravel()}).astype(np.float64).reshape(2, 4, 8)
    for i in range(2):
        assert _rel(x @ t[i, :3, :K].T, O.matmul(x, bm[i].astype(np.float64))) <= 1e-12


def test_clip_embed_reference_agrees_with_the_oracle_embedding():
    d, ops = _case("clip_d768")
    B, T, V, D = 3, 5, 11, 768
    tok = np.clip(ops["X"], 0, V - 1)
    want = O.embedding(tok, ops["W"].reshape(V, D).astype(np.float32)).reshape(B, T, D) + ops["BIAS"].reshape(1, T, D)
    with np.errstate(over="ignore"):
        assert np.array_equal(E.expected(d, ops).view(np.uint16), want.astype(np.float16).ravel().view(np.uint16))


# ---- value-coded inputs ----------------------------------------------------------------------------------------------------------------
def test_movement_inputs_are_distinct_and_carry_the_rounding_edges():
    for name, d, kind, _ in SWEEP:
        if E.mode_of(d) not in E.EXACT or kind:
            continue
        ops = E.make_inputs(d, SEED, kind)
        for s in ("X", "W", "BIAS"):
            if s in ops and ops[s].dtype != np.int32:
                v = ops[s].astype(np.float64)
                v = v[~np.isnan(v)]
                assert np.unique(v).size == v.size, f"{name}: {s} holds equal values"
    x = E.coded32(1344)
    h = x.astype(np.float64)
    with np.errstate(over="ignore"):
        r16 = x.astype(np.float16).astype(np.float64)
    assert (np.abs(h) > 65504).sum() >= 4 and np.isinf(r16).sum() >= 4                     # beyond fp16
    assert ((np.abs(h) < 2.0 ** -14) & (h != 0)).sum() >= 5                                # subnormal in fp16
    ulp = 2.0 ** -10
    assert (np.abs(np.abs(h - r16) - ulp / 2) < 1e-12).sum() >= 3                          # ties at 1 + k 2^-11


# ---- the emulation inside the bound; the cap --------------------------------------------------------------------------------------------
HALF = ("SMALL_LINEAR",)


@pytest.mark.parametrize("name,d,kind,expect", SWEEP, ids=[s[0] for s in SWEEP])
def test_emulation_stays_inside_the_bound(name, d, kind, expect):
    """Worst error / bound <= 0.5 wherever the bound is more than the result's own last roundings: for SMALL_LINEAR, and on the fp32 value
    before the fp16 store for GEGLU_ERF.  The bounds of QUICK_GELU (before its store), TIME_EMBEDDING, UNARY and ENCODER_SAMPLE are a count of the last
    one to four roundings of the result, each taken at its half-ulp worst case: a faithfully computed value may sit near the bound
    itself (a correctly rounded time embedding reaches 0.99 of it), so there the emulation is held to the bound.  The movement modes are
    bit-exact (0)."""
    m = E.mode_of(d)
    ops = E.make_inputs(d, SEED, kind)
    out = E.emulate(d, ops)
    fails, ratio = E.check(d, ops, out)
    assert not fails, fails
    assert E.nonfinite_expected(d, ops) == expect["NONFINITE"]
    if m in HALF or m in E.EXACT:
        assert ratio <= 0.5, ratio
    elif m in ("GEGLU_ERF", "QUICK_GELU"):
        ref, share = E.fp32_share(d, ops)
        raw = E.emulate(d, ops, raw=True).astype(np.float64).reshape(ref.shape)
        assert (np.abs(raw - ref) <= (0.5 if m == "GEGLU_ERF" else 1.0) * share).all()
    if m == "SMALL_LINEAR":
        n, worst = E.cap_violations(d, ops)
        assert n == 0, f"bound above 2^-10 (|ref| + 1) at {n} elements (worst {worst:.3g} x cap)"


def test_small_linear_cap_is_what_the_issue_measured():
    d, ops = _case("sl_lds_160k")
    assert 2.0 ** -12.2 < E.cap_violations(d, ops)[1] * 2.0 ** -10 < 2.0 ** -11.2     # about 2^-11.6 at B = 16, K = 2560


# ---- seeded defects ----------------------------------------------------------------------------------------------------------------
MUTATIONS = [
    ("a lane's last chunk dropped", "last_chunk", "sl_k1288_b3_n17_silu0"),
    ("a lane's last chunk dropped", "last_chunk", "sl_k1288_b3_n17_silu1"),
    ("the second K pass dropped", "second_pass", "sl_k2056_b3_n17_silu0"),
    ("the second K pass dropped", "second_pass", "sl_k2560_b3_n17_silu1"),
    ("row N - 1 written for n >= N", "row_clamp", "sl_pitches_silu0"),
    ("SiLU skipped", "no_silu", "sl_b3_k320_n48_silu1"),
    ("bias of the wrong column", "bias_col", "sl_n17_b2_k128"),
    ("b and NB confused: sample B - 1 taken from sample 0", "b_nb", "sl_b3_k320_n48_silu0"),
    ("tap (kh, kw) transposed", "tap_transposed", "im2col_c3_5x3_b1_s1"),
    ("the edge test off by one", "edge_off_by_one", "im2col_c4_2x5_b3_svae"),
    ("tap-major and channel-major swapped", "tap_channel_swapped", "pack_conv_k3"),
    ("interleave halves swapped", "halves_swapped", "pack_linear_il1"),
    ("interleave halves swapped", "halves_swapped", "pack_bias_il1"),
    ("position taken as row / T", "pos_row_div", "clip_d1032"),
    ("sin / cos halves swapped", "sincos_swapped", "temb_t980_b3"),
    ("row b taken from t[0]", "row_t0", "temb_array_b16"),
    ("(a, gate) swapped", "swap_a_gate", "geglu_random"),
    ("tanh-GELU in place of erf-GELU", "tanh_gelu", "geglu_all_gates"),
]


@pytest.mark.parametrize("what,mut,name", MUTATIONS, ids=[f"{m[1]}-{m[2]}" for m in MUTATIONS])
def test_seeded_defect_is_rejected(what, mut, name):
    d, ops = _case(name)
    fails, _ = E.check(d, ops, E.emulate(d, ops))
    assert not fails, f"the unmutated emulation must pass: {fails}"
    fails, ratio = E.check(d, ops, E.emulate(d, ops, mut=mut))
    assert fails and ratio > 2, f"{what}: not rejected (worst error {ratio:.3g} x bound)"
