"""No GPU: tests/chain_ref.py - the fp64 reference, the float32 emulation, the checks and their measured limits for the fused
attention-block head / tail kernels of csrc/kernels_chain.hip - is itself tested.  The reference agrees with a composition of the
oracle's own ops in float64 (the interleave of W1 / b1 included); the operand extents agree with tsd_debug_chain_run's sizing-only mode
on the whole sweep and what cannot be sized is refused; the limits written into chain_ref.py are recomputed from the emulation alone,
which stays below half of each margin on every sweep case; every seeded defect of the emulation is rejected on a named sweep case the
GPU test runs too, by the check named here."""
import numpy as np
import pytest

import chain_ref as R
import replay
from oracle import ops as O


def _size(d, n=None):
    info = np.full(R.CI["COUNT"], -1, np.int64)
    rc, ext = replay.size("tsd_debug_chain_run", d, n, info)
    return rc, {s: int(ext[R.CO[s]]) for s in R.INPUTS + R.OUTPUTS}, info


# ---- the reference against the oracle ----------------------------------------------------------------------------------------------
def test_tail_reference_is_the_oracles_composition():
    d = R.tail_desc(2, 64, T=77, **R.PITCHED)
    ops = R.make_inputs(d, "flat", seed=3)
    L = {k: v.astype(np.float64) for k, v in R.unpack(d, ops).items()}
    B, S, T = 2, 64, 77
    eps, s32 = float(np.float32(1e-5)), float(replay.bits_f32(R.F(d, "SCALE")))
    w1 = np.concatenate([L["W1"][0::2], L["W1"][1::2]])           # the reference order: all "a" rows, then all gates
    b1 = np.concatenate([L["B1"][0::2], L["B1"][1::2]])
    tok2 = O.linear(L["AO"], L["WSO"], L["BSO"]) + L["TOK"]
    q = O.linear(O.layer_norm(tok2, eps), L["WQ"])
    k_fix = s32 * np.sqrt(float(R.HD))                            # the oracle scales by 1 / sqrt(40) in float64, the launch by its float32
    attn = np.concatenate([O.attention_core(q[b * S:(b + 1) * S], L["KC"][b] * k_fix, L["VT"][b][:, :T].T, R.HEADS) for b in range(B)])
    tok3 = tok2 + O.linear(attn, L["WCO"], L["BCO"])
    a, g = np.split(O.linear(O.layer_norm(tok3, eps), w1, b1), 2, axis=-1)
    tok4 = tok3 + O.linear(a * O.gelu_tanh(g), L["W2"], L["B2"])
    want = L["X"] + O.linear(tok4, L["WOUT"], L["BOUT"])
    got = R.reference(d, ops)["OUT"]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_head_reference_is_the_oracles_composition():
    """x is m +- a per group with as many + as -, a a power of two: mean m and sigma a exactly, so the GIVEN fp32 pairs (m, 1 / a) are the
    oracle's own statistics (its eps set to 0) and the two can be compared to 1e-12."""
    B, S = 2, 64
    d = R.head_desc(B, S, ld_vt=72, **R.HEAD_PITCHED)
    r = np.random.default_rng(11)
    L = R.make_logical(d, "flat", seed=3)
    m = np.round(4 * r.standard_normal((B, 1, 32, 1))) / 4
    a = 2.0 ** r.integers(-2, 2, (B, 1, 32, 1))
    sign = np.stack([r.permutation(np.repeat([1.0, -1.0], S * 5)).reshape(S, 10) for _ in range(B * 32)]).reshape(B, 32, S, 10).transpose(0, 2, 1, 3)
    x = (m + a * sign).reshape(B * S, R.C)
    L["X"], L["GN_STATS"] = x, np.stack([m[:, 0, :, 0], 1.0 / a[:, 0, :, 0]], axis=-1)
    ops = R.pack(d, L)
    assert np.array_equal(R.unpack(d, ops)["X"].astype(np.float64), x)
    L = {k: v.astype(np.float64) for k, v in R.unpack(d, ops).items()}
    gn = np.concatenate([O.group_norm(np.ascontiguousarray(x[b * S:(b + 1) * S].T).reshape(R.C, S, 1), 32, eps=0.0).reshape(R.C, S).T for b in range(B)])
    tok = O.linear(gn, L["WC"], L["B_IN"])
    qkv = O.linear(O.layer_norm(tok, float(np.float32(1e-5))), L["WIN"])
    got = R.reference(d, ops)
    for s, want in (("HTOK", tok), ("QK", qkv[:, :640]), ("HVT", qkv[:, 640:])):
        assert np.abs(got[s] - want).max() <= 1e-12 * np.abs(want).max(), s
    # and the statistics make_inputs passes are those of x
    st = R.gn_stats_of(x, B, S, eps=0.0).astype(np.float64)
    assert np.array_equal(st, L["GN_STATS"].reshape(B, 32, 2))


# ---- sizing --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,kind", R.SWEEP, ids=R.NAMES)
def test_sizing_call_agrees_with_chain_ref(tsd_mod, name, d, kind):
    rc, ext, info = _size(d)
    assert rc == 0, tsd_mod._lib.lib().tsd_last_error().decode()
    assert ext == R.extents(d)
    assert (info[:R.CI["COUNT"]] == 0).all()


def test_descriptors_that_cannot_be_sized_are_refused(tsd_mod):
    for good in (R.tail_desc(3, 64, **R.PITCHED), R.head_desc(3, 64, ld_vt=72, **R.HEAD_PITCHED)):
        assert _size(good)[0] == 0
        assert _size(good, n=R.COUNT - 1)[0] != 0
        bad_fields = [("VERSION", 7), ("MODE", 5), ("B", 0), ("S", 0), ("C", 0), ("D", 0), ("HEADS", -1), ("LD_X", 0), ("B", 1 << 20)]
        bad_fields += [("T", -1), ("GN", 2), ("LDK", 0), ("SKB", 10), ("SVTB", 10), ("LDW_2", 0)] if R.is_tail(good) else [("S_VT", 10), ("LD_QK", 0)]
        for f, v in bad_fields:
            bad = good.copy()
            bad[R.CD[f]] = v
            assert _size(bad)[0] != 0, f
    # what the launchers refuse is sized
    for d in (R.tail_desc(1, 96), R.tail_desc(1, 32), R.tail_desc(1, 64, T=0), R.tail_desc(1, 64, T=81, ldvt=88), R.tail_desc(1, 64, ld=(324, 320, 320, 320)),
              R.tail_desc(1, 64, ld=(320, 320, 320, 312)), R.tail_desc(1, 64, T=77, ldvt=72), R.tail_desc(1, 64, C=640), R.head_desc(1, 128, ld_vt=64),
              R.head_desc(1, 64, C=640), R.tail_desc(1, 64, ldw=(312, 320, 320, 320, 1280, 320))):
        rc, ext, _ = _size(d)
        assert rc == 0 and ext == R.extents(d)


# ---- the measured limits ----------------------------------------------------------------------------------------------------------------
def test_limits_are_what_the_formulas_give():
    assert R.K_ELEM == 2 * R.MEASURED_EXCESS
    assert R.L_STAT == {k: min(1 + 3 * v, 2.0) for k, v in R.MEASURED_SPREAD.items()} and max(R.L_STAT.values()) <= 2.0


def test_written_figures_are_the_measured_ones():
    """The constants are the maxima over the sweep rounded UP to two digits: never below what the emulation gives, never 10 % above."""
    ex, spread = R.measure_limits()
    print(f"[chain] measured over the sweep: excess {ex:.4f} spreads " + " ".join(f"{k} {v:.5f}" for k, v in spread.items()))
    assert 0.9 * R.MEASURED_EXCESS <= ex <= R.MEASURED_EXCESS
    for k, v in spread.items():
        assert 0.9 * R.MEASURED_SPREAD[k] <= v <= R.MEASURED_SPREAD[k], k


@pytest.mark.parametrize("name", R.NAMES)
def test_emulation_alone_stays_below_half_of_each_margin(name):
    """The figures the limits are made of, recomputed: the emulation at the other accumulation orders against the one at 32."""
    d, kind, ops, ref, emu = R.case(name)
    ex, spread = R.figures(name)
    print(f"[chain] {name}: excess {ex:.2f} spreads " + " ".join(f"{k} {v:.4f}" for k, v in spread.items()))
    assert ex <= R.K_ELEM / 2, f"{name}: excess {ex:.3f} above K_ELEM / 2"
    for k, v in spread.items():
        assert v <= (R.L_STAT[k] - 1) / 2, f"{name}: {k} spread {v:.4f} above half of the margin of L = {R.L_STAT[k]}"
    orders = R.orders_of(name)
    for c in sorted({orders[0], orders[-1]}):
        out, _ = R.emulate(d, ops, chunk=c)
        fails, worst = R.check(d, ops, out, emu, ref, k_elem=R.K_ELEM / 2, l_stat={k: 1 + (v - 1) / 2 for k, v in R.L_STAT.items()})
        assert not fails, f"{name} at chunk {c}: {fails}"
    fails, _ = R.check(d, ops, emu[0], emu, ref)
    assert not fails, fails


# ---- seeded defects ----------------------------------------------------------------------------------------------------------------------
ALL = ("elem", "whole", "rows", "cols", "tiles")
DEFECT_CASES = {   # mutation: ((sweep case the GPU test runs too, the checks that must reject it), ...)
    "drop_last_key": (("tail/B1_S64", ALL), ("tail/T7", ALL), ("tail/T64", ALL), ("tail/T80", ALL)),
    "admit_key_T": (("tail/T7", ALL), ("tail/T33", ALL), ("tail/T64", ALL), ("tail/B1_S64", ALL)),
    "mask_fragment4_only": (("tail/T7", ALL), ("tail/T33", ALL)),
    "scale_without_log2e": (("tail/B1_S64", ALL), ("tail/peaked", ALL)),
    "ln_per_column_wave": (("tail/B1_S64", ALL), ("tail/ln_offset", ALL)),
    "ln_merge_without_between_term": (("tail/ln_offset", ALL), ("tail/B1_S64", ALL)),
    "geglu_halves_swapped": (("tail/B1_S64", ALL), ("tail/wide_gates", ALL)),
    "geglu_chunk_repeated": (("tail/B1_S64", ALL), ("tail/wide_gates", ALL)),
    "no_b2": (("tail/B1_S64", ALL),),
    "b1_not_interleaved": (("tail/B1_S64", ALL), ("tail/wide_gates", ALL)),
    "long_residual_from_tok": (("tail/B1_S64", ALL), ("tail/B3_S64_pitched", ALL)),
    "context_of_sample_0": (("tail/B3_S64_pitched", ALL), ("tail/B2_S128_gn", ALL)),          # needs B > 1
    "wco_ktiles_3_4_swapped": (("tail/B1_S64", ALL), ("tail/equal_keys", ALL)),
    "gn_slab_of_64_rows": (("tail/B1_S64_gn", ("gn",)), ("tail/B2_S128_gn", ("gn",))),
    "gn_group_of_20": (("head/group_means", ALL), ("head/B3_S64_pitched", ALL)),
    "stats_of_sample_0": (("head/B3_S64_pitched", ALL), ("head/group_means", ALL)),           # needs B > 1
    "k_from_wq": (("head/B1_S64", ALL),),
    "v_rows_in_qk_order": (("head/B1_S64", ALL), ("head/B3_S64_pitched", ALL)),
    "vt_second_tile_at_column_0": (("head/B2_S128", ALL), ("head/B1_S192", ALL)),               # needs S > 64
}


def test_every_mutation_has_its_cases():
    assert sorted(DEFECT_CASES) == sorted(R.MUTATIONS)


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_seeded_defect_is_rejected(mut):
    for name, kinds in DEFECT_CASES[mut]:
        d, _, ops, ref, emu = R.case(name)
        assert not R.check(d, ops, emu[0], emu, ref)[0], f"{name}: the unmodified emulation fails"
        bad, _ = R.emulate(d, ops, mut=mut)
        fails, worst = R.check(d, ops, bad, emu, ref)
        assert fails, f"{mut} passes on {name}"
        for k in kinds:
            assert not worst[k] <= 1.0, f"{mut} on {name}: the {k} check passes (ratio {worst[k]:.3f})"


def test_defects_that_need_more_than_one_sample_or_workgroup_change_nothing_without():
    for mut, name in (("context_of_sample_0", "tail/B1_S64"), ("stats_of_sample_0", "head/B1_S64"), ("vt_second_tile_at_column_0", "head/B1_S64")):
        d, _, ops, _, emu = R.case(name)
        bad, _ = R.emulate(d, ops, mut=mut)
        assert all(np.array_equal(bad[s].view(np.uint16), emu[0][s].view(np.uint16)) for s in R.fp16_outputs(d)), (mut, name)


def test_finite_pad_columns_do_not_change_the_emulation_and_the_fill_does():
    """V^T columns [T, round_up(T, 8)) meet P = 0: any finite content gives the same bits; the NaN fill there would reach every output."""
    for T in R.PAD_T:
        d = R.tail_desc(1, 64, T=T, ldvt=88)
        z, f = R.make_inputs(d, "flat", seed=R.SEED, pad=0.0), R.make_inputs(d, "flat", seed=R.SEED, pad=R.pad_fill(d))
        assert not np.array_equal(z["VT"].view(np.uint16), f["VT"].view(np.uint16))
        y0, y1 = R.emulate(d, z)[0]["OUT"], R.emulate(d, f)[0]["OUT"]
        assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16))
