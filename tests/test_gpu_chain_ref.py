"""GPU: the fused attention-block kernels - attn_chain_kernel<KIND_HEAD>, attn_chain_kernel<KIND_TAIL> and the two weight-stream packers
(csrc/kernels_chain.hip) - held to an fp64 reference element-wise (tests/chain_ref.py) through tsd_debug_chain_run: chosen operand
bits in the device layout, NaN-guarded operands (pitch gaps, K rows >= T, V^T columns >= round_up(T, 8)), one, two and three workgroups
per sample, B > 1 at S = 64, wider pitches with gaps between the samples, every key-fragment and chunk edge of T, the input shapes of
chain_ref (flat, peaked scores, equal keys, a LayerNorm offset per column quarter, wide gates, distinct GroupNorm groups), the output's
GroupNorm partials off and on, 264 workgroups (a second round on every CU), finite garbage in the V^T pad columns, repeatability,
sample independence, the head feeding the tail, and the documented refusals.  Every case asserts the status, that the kernel ran, that
no guard or pitch-gap element was written and every check of chain_ref.check; it prints the worst ratio of each check to its limit.

Worst ratio to the limit seen on an MI355X (profiles/r08_gpu_chain_ref.log) - element, whole, rows, columns, tiles; GroupNorm partials where emitted:
tail shapes 0.401 0.985 0.564 0.573 0.797, partials 0.007; T sweep 0.410 0.988 0.588 0.630 0.800; input kinds 0.432 0.985 0.556 0.557 0.814;
tail, 264 workgroups 0.440 0.984 0.593 0.504 0.832, partials 0.009; head shapes 0.493 0.984 0.521 0.560 0.759; head, 264 workgroups 0.484
0.984 0.547 0.501 0.772; V^T pad columns 0.412 0.986 0.558 0.574 0.781; head feeding the tail 0.369 0.984 0.530 0.534 0.774, partials 0.007.
The emulation against itself gives 0.36 0.98 0.50 0.50 0.74."""
import numpy as np
import pytest

import chain_ref as R
import replay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx, tsd_mod):
    c = tsd_mod.Context(gpu_ctx.device)
    yield c
    c.close()


def run(ctx, d, ops):
    """(status, {output: flat array}, info {CHANGED, RAN})."""
    rc, outs, info = replay.run("tsd_debug_chain_run", ctx, d, ops, R.CO, R.INPUTS, R.OUTPUTS, R.dtype_of, R.extents)
    return rc, outs, {k: int(info[v]) for k, v in R.CI.items() if k != "COUNT"}


def verify(ctx, name, d, ops, ref=None, emu=None):
    """Run d and hold it to the reference; returns the outputs."""
    rc, outs, info = run(ctx, d, ops)
    assert rc == 0, f"{name}: status {rc}: {replay.lib().tsd_last_error().decode()}"
    assert info["RAN"] == 1, f"{name}: the kernel was not launched"
    assert info["CHANGED"] == 0, f"{name}: {info['CHANGED']} guard / pitch-gap elements written"
    for s in R.fp16_outputs(d):
        replay.assert_gaps_hold_fill(outs[s], R.index(d, s), f"{name}: {s}")
    emu = emu if emu is not None else R.emulate(d, ops)
    fails, worst = R.check(d, ops, outs, emu, ref, changed=info["CHANGED"])
    print(f"[chain] {name}: worst ratio to the limit " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not fails, f"{name}: " + "; ".join(fails)
    return outs


def same_bits(a, b):
    return all(np.array_equal(a[s].view(np.uint8), b[s].view(np.uint8)) for s in a)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_chain_kernel_matches_the_fp64_reference(ctx, name):
    d, kind, ops, ref, emu = R.case(name)
    assert np.isnan(ops["X"]).any() or R.F(d, "LD_X") == R.C        # (the pitched cases carry the fill in their gaps)
    outs = verify(ctx, name, d, ops, ref, emu)
    rc, again, info = run(ctx, d, ops)
    assert rc == 0 and info["RAN"] == 1 and same_bits(outs, again), f"{name}: a second run gave other bits"


# ---- V^T pad columns ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.PAD_T)
def test_finite_pad_columns_of_vt_do_not_change_a_bit(ctx, T):
    """V^T columns [T, round_up(T, 8)) reach the P.V MFMA with P = 0: any finite content gives the same bits.  Columns beyond, K rows >= T
    and every pitch gap hold the NaN pattern in both runs and are never read."""
    d = R.tail_desc(2, 64, T=T, ldvt=88, krows=80, gap=16)
    z, f = R.make_inputs(d, "flat", seed=R.SEED, pad=0.0), R.make_inputs(d, "flat", seed=R.SEED, pad=R.pad_fill(d))
    assert R.tv_of(d) > T and not np.array_equal(z["VT"].view(np.uint16), f["VT"].view(np.uint16))
    assert np.isnan(z["VT"]).any() and np.isnan(z["KC"]).any()
    ref, emu = R.reference(d, z), R.emulate(d, z)
    y0 = verify(ctx, f"pad/T{T}/zero", d, z, ref, emu)
    y1 = verify(ctx, f"pad/T{T}/60000", d, f, ref, emu)
    assert same_bits(y0, y1), f"T = {T}: the V^T pad columns reached the output"


# ---- samples are independent ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,one", [("tail/B3_S64_pitched", R.tail_desc(1, 64, **R.PITCHED)),
                                      ("head/B3_S64_pitched", R.head_desc(1, 64, ld_vt=72, **R.HEAD_PITCHED))], ids=("tail", "head"))
def test_sample_1_of_three_equals_a_run_on_its_operands_alone(ctx, name, one):
    d, kind, ops, ref, emu = R.case(name)
    rc, outs, info = run(ctx, d, ops)
    assert rc == 0 and info["RAN"] == 1
    L = R.sample_logical(d, R.unpack(d, {s: ops[s] for s in ops}), 1)
    rc, alone, info = run(ctx, one, R.pack(one, L))
    assert rc == 0 and info["RAN"] == 1 and info["CHANGED"] == 0
    for s in R.fp16_outputs(d):
        y3, y1 = R.token_major(d, s, outs[s]), R.token_major(one, s, alone[s])
        assert np.array_equal(y3[64:128].view(np.uint16), y1.view(np.uint16)), f"{s}: sample 1 depends on its neighbours"


# ---- the head feeds the tail -------------------------------------------------------------------------------------------------------------
def test_head_output_feeds_the_tail(ctx):
    """The layouts one kernel writes and the other reads: the head's tok (and its x as the long residual) into the tail, with a chosen ao."""
    dh, _, oh, refh, emuh = R.case("head/B3_S64_pitched")
    got = verify(ctx, "chained/head", dh, oh, refh, emuh)
    dt = R.tail_desc(3, 64, gn=1, **dict(R.PITCHED, ld=(328, R.F(dh, "LD_TOK"), R.F(dh, "LD_X"), 352)))
    ops = R.make_inputs(dt, "flat", seed=R.SEED + 1)
    assert ops["TOK"].size == got["HTOK"].size and ops["X"].size == oh["X"].size
    ops["TOK"], ops["X"] = got["HTOK"], oh["X"]           # flat arrays in the device layout, fill in the gaps included
    verify(ctx, "chained/tail", dt, ops)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _refusals():
    return [
        ("tail_S96", R.tail_desc(1, 96)), ("head_S96", R.head_desc(1, 96, ld_vt=96)),
        ("tail_M32", R.tail_desc(1, 32)), ("head_M32", R.head_desc(1, 32)),
        ("T0", R.tail_desc(1, 64, T=0)), ("T81", R.tail_desc(1, 64, T=81, ldvt=88)),
        ("ld_ao_324", R.tail_desc(1, 64, ld=(324, 320, 320, 320))), ("ld_out_312", R.tail_desc(1, 64, ld=(320, 320, 320, 312))),
        ("ldvt_below_round_up_T", R.tail_desc(1, 64, T=77, ldvt=72)),
        ("head_ld_vt_below_S", R.head_desc(1, 128, ld_vt=64)),
        ("tail_C640", R.tail_desc(1, 64, C=640, D=80)), ("head_C640", R.head_desc(1, 64, C=640, D=80)),
        ("tail_weight_pitch_312", R.tail_desc(1, 64, ldw=(320, 320, 312, 320, 1280, 320))),
    ]


def _refused(ctx, name, d):
    r = np.random.default_rng(3)
    ext = R.extents(d)
    ops = {s: r.standard_normal(ext[s]).astype(R.dtype_of(s)) for s in R.INPUTS if ext[s]}
    rc, outs, info = run(ctx, d, ops)
    assert rc != 0, f"{name} was not refused"
    assert info == {"CHANGED": 0, "RAN": 0}, info
    replay.assert_untouched(outs, name)


@pytest.mark.parametrize("name,d", _refusals(), ids=[r[0] for r in _refusals()])
def test_refused_launches_leave_the_outputs_untouched(ctx, name, d):
    _refused(ctx, name, d)


@pytest.mark.parametrize("d", [R.tail_desc(1, 64, gn=1), R.head_desc(1, 64)], ids=("tail", "head"))
def test_fused_path_switched_off_is_refused(ctx, d):
    lib = replay.lib()
    was = lib.tsd_debug_set_fused_attention(ctx.h, 0)
    try:
        _refused(ctx, "fused_off", d)
    finally:
        lib.tsd_debug_set_fused_attention(ctx.h, was)
    ops = R.make_inputs(d, "flat", seed=1)
    rc, outs, info = run(ctx, d, ops)
    assert rc == 0 and info["RAN"] == 1, "the switch was not restored"
