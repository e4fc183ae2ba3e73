"""No GPU: what the head-dimension-64 attention core rests on.  tests/attn64_ref.py - the fp64 reference, the no-ones-row bound at dpad = 64,
the exact-repeat prediction and the numpy emulation of flash_attn_kernel<64, 1> - is itself tested: the reference agrees with the
oracle's attention; tsd_debug_attn_run's sizing-only mode sizes version-2 descriptors as the module does and names TSD_AK_64, and treats a
version-1 descriptor at d = 64 as it always did; the emulation stays inside the bound on every sweep input the GPU test runs and takes the
exact repeat where the prediction says it must; every seeded defect is rejected on such an input.  And the untouched ground: every row of
csrc/isa_contract.json that existed before the d = 64 kernel is what it was (tests/golden/isa_contract_rows_before_d64.json), the new
kernel has a row without scratch, and the existing enum values kept their numbers."""
import hashlib
import json
import os

import numpy as np
import pytest

import attn64_ref as R
import attn_ref as A
import replay
from oracle import ops as O

SWEEP = R.sweep()
NAMES = [s[0] for s in SWEEP]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _size(d, n=None):
    info = np.full(A.AI["COUNT"], -1, np.int64)
    rc, ext = replay.size("tsd_debug_attn_run", d, n, info)
    return rc, {s: int(ext[A.AO[s]]) for s in A.INPUTS + ("O",)}, {k: int(info[v]) for k, v in A.AI.items() if k != "COUNT"}


# ---- the reference against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Sq,Sk", [(5, 64, 77), (20, 33, 129)])
def test_reference_agrees_with_the_oracle_attention(H, Sq, Sk):
    d = R.attn_desc(1, H, Sq, Sk)
    ops = R.make_inputs(d, "flat", seed=3)
    q, k, v, _ = (x.astype(np.float32) for x in A.unpack_inputs(d, ops))
    tok = lambda x: np.ascontiguousarray(x[0].transpose(1, 0, 2).reshape(x.shape[2], H * 64))
    want = O.attention_core(tok(q), tok(k), tok(v), H).astype(np.float64)
    ref, bd = R.reference(d, ops)
    assert np.abs(tok(ref) - want).max() <= 2e-5 * (1 + np.abs(want).max())   # the oracle works in fp32
    assert (bd < 1e-2 * (1 + np.abs(ref))).all()


# ---- sizing, the dispatcher, the two descriptor versions -------------------------------------------------------------------------------
def test_enum_values_kept_their_numbers_and_the_new_ones_follow():
    assert A.AK == {"NONE": 0, "40_1": 1, "40_2": 2, "40_8W": 3, "80": 4, "160": 5, "64": 6}
    assert A.AD_VERSION == 1 and R.AD_VERSION_2 == 2


@pytest.mark.parametrize("name,d,kind", SWEEP[::5], ids=NAMES[::5])
def test_sizing_call_agrees_with_attn64_ref(tsd_mod, name, d, kind):
    rc, ext, info = _size(d)
    assert rc == 0, replay.lib().tsd_last_error().decode()
    assert ext == A.extents(d)
    p = R.plan(d)
    assert {k: info[k] for k in p} == p
    assert info["CHANGED"] == 0 and info["EXACT_WGS"] == 0


def test_dispatcher_takes_the_d64_kernel_at_every_shape_and_never_looks_at_the_batch(tsd_mod):
    for B, H, Sq, Sk in ((2, 5, 4096, 4096), (1, 5, 4096, 4096), (2, 5, 9216, 9216), (2, 10, 1024, 1024), (2, 20, 256, 256), (2, 5, 4096, 77), (7, 20, 64, 77)):
        for force in (0, 1, 2, 3):      # the d = 40 variant switch does not reach d = 64
            d = R.attn_desc(B, H, Sq, Sk, dense=True, kernel=force)
            rc, _, info = _size(d)
            assert rc == 0 and info["KERNEL"] == A.AK["64"] and info["DIAG"] == (1 if Sq == Sk else 0) and info["XCD_MAP"] == 0, (B, H, Sq, Sk, info)


def test_version_1_descriptor_keeps_its_behaviour_at_d64_and_version_2_refuses_what_it_must(tsd_mod):
    v1 = R.attn_desc(1, 1, 8, 16, version=1)
    assert np.array_equal(v1, A.attn_desc(1, 1, 64, 8, 16))
    rc, ext, info = _size(v1)
    assert rc == 0 and ext == A.extents(v1) and all(v == 0 for v in info.values()), info       # sized, no kernel named
    rc, ext, info = _size(R.attn_desc(1, 2, 8, 16, hd=48))                                      # d = 48: sized, left to the launcher
    assert rc == 0 and info["KERNEL"] == 0
    for ver in (0, 3, 7):
        assert _size(R.attn_desc(1, 5, 8, 16, version=ver))[0] != 0, ver
    good = R.attn_desc(2, 5, 33, 77)
    assert _size(good)[0] == 0 and _size(good, n=A.COUNT - 1)[0] != 0
    for f, v in (("B", 0), ("LDQ", 5 * 64 - 8), ("LDVT", 76), ("KERNEL", 4), ("DIAG", 2)):
        bad = good.copy()
        bad[A.AD[f]] = v
        assert _size(bad)[0] != 0, f
    for name, d, _ in A.sweep()[::17]:      # version-1 descriptors of the other head dimensions: the plan attn_ref states
        rc, ext, info = _size(d)
        p = A.plan(d)
        assert rc == 0 and ext == A.extents(d) and {k: info[k] for k in p} == p, name


# ---- the emulation inside the bound, the prediction ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_emulation_stays_inside_the_bound(name):
    d, kind, ops, ref = R.case(name)
    if kind != "onehot":
        assert R.well_conditioned(d, ops)
    y, repeats = R.emulate(d, ops)
    fails, ratio = R.check(d, ops, y, ref=ref)
    assert not fails and ratio <= 1.0, f"{name}: {fails}"
    pr = R.predict_repeat(d, ops)
    assert (pr == 1).sum() <= repeats <= (pr >= 0).sum(), f"{name}: {repeats} repeats, prediction {pr.tolist()}"
    assert np.array_equal(np.isnan(y), np.isnan(A.pack_output(d, np.zeros(ref[0].shape))))


def test_prediction_covers_must_must_not_and_the_edge():
    for name, want in (("edge_lo", -1), ("edge_hi", 1), ("spike_t9of10", 1), ("spike_t4of10", 1), ("rising", 1), ("spike", 1), ("subtail", -1),
                       ("sk641", -1), ("self320/diag1", -1), ("self320/diag0", 1)):
        d, _, ops, _ = R.case(name)
        assert (R.predict_repeat(d, ops) == want).all(), name


def test_bound_needs_its_no_ones_row_term():
    """`pbias`: every key but one carries the same P with the same positive fp16 rounding error.  With a ones row that error would cancel
    between numerator and denominator; here the denominator sums the unrounded P, so it reaches the output - the emulation's error uses a
    good part of the h sum_k w_k |v_kj| term the no-ones-row form adds, and stays inside the bound."""
    d, _, ops, (o, bd) = R.case("pbias")
    y, _ = R.emulate(d, ops)
    err = np.abs(A.unpack_output(d, y).astype(np.float64) - o)
    assert (err <= bd).all() and (err / bd).max() > 0.3


# ---- seeded defects ----------------------------------------------------------------------------------------------------------------
DEFECT_CASES = {   # every one a case tests/test_gpu_attn64.py runs on the device
    "drop_last_key": ("sk77", "sk641", "sk1"),
    "admit_masked_key": ("sk77", "sk4"),
    "scale_sqrt80": ("sq129", "sk577"),
    "v_swap_bits23": ("sk64", "sk577"),
    "head_offset_b": ("sq33", "h20/sq129_sk65"),
    "no_alpha": ("rising", "edge_hi", "spike_t9of10"),
    "flush_subnormal_p": ("subtail",),
    "pad_weight_2m24": ("pad_sk7", "pad_sk193"),
    "skip_repeat": ("spike_t9of10", "spike", "edge_hi"),
    "early_look_drops_tail": ("sk577", "sk641", "spike_t9of10"),
}


@pytest.mark.parametrize("mut", sorted(DEFECT_CASES))
def test_seeded_defect_is_rejected(mut):
    for name in DEFECT_CASES[mut]:
        if name.startswith("pad_"):
            d = dict(R.pad_sweep())[name]
            ops = R.make_inputs(d, "flat", seed=7, pad=A.pad_fill(d))
            ref = R.reference(d, ops)
        else:
            d, _, ops, ref = R.case(name)
        good, _ = R.emulate(d, ops)
        assert not R.check(d, ops, good, ref=ref)[0], f"{name}: the unmodified emulation fails"
        bad, _ = R.emulate(d, ops, mut=mut)
        fails, ratio = R.check(d, ops, bad, ref=ref)
        assert fails and ratio > 1.0, f"{mut} passes on {name} (worst error / bound {ratio:.3f})"


def test_every_mutation_has_a_case():
    assert set(DEFECT_CASES) == set(R.MUTATIONS)


# ---- the untouched ground ----------------------------------------------------------------------------------------------------------
def test_isa_contract_rows_of_every_earlier_kernel_are_unchanged_and_the_new_kernel_has_one():
    table = json.load(open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "csrc", "isa_contract.json")))
    table.pop("_meta")
    rows = {f"{f}::{k}": hashlib.sha256(json.dumps(r, sort_keys=True).encode()).hexdigest()[:24] for f, ft in table.items() for k, r in ft.items()}
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_contract_rows_before_d64.json")))
    assert len(before) == 156
    changed = sorted(k for k, v in before.items() if rows.get(k) != v)
    assert not changed, f"rows of earlier kernels changed or vanished: {changed}"
    new = table["kernels_attn"]["_Z17flash_attn_kernelILi64ELi1EEv5AttnK"]
    assert "scratch=0" in new["regs"] and "vgpr_spill=0" in new["regs"] and "counted=0" in new["waits"], new
    vgpr = int(new["regs"].split("vgpr=")[1].split()[0])
    assert vgpr <= 168, f"{vgpr} VGPRs: three workgroups per CU (TSD_ATTN64_WGS) need at most 168"


# ---- the SD-2.x model kinds: inventory, refusals, key maps (host code only) ------------------------------------------------------------
def test_reserved_and_unknown_kinds_are_refused(tsd_mod):
    lib = tsd_mod._lib.lib()
    for kind in (0, 12, 13, 14, 15, 18, 19):
        assert lib.tsd_model_param_count(kind) == tsd_mod._lib.TSD_E_ARG, kind
    for kind in list(range(1, 12)) + [16, 17]:
        assert lib.tsd_model_param_count(kind) > 0, kind
    assert tsd_mod.model.KINDS["diffusion_sd2"] == 16 and tsd_mod.model.KINDS["clip_sd2"] == 17
    hdr = replay.header()
    assert "TSD_MODEL_DIFFUSION_SD2 = 16" in hdr and "TSD_MODEL_CLIP_SD2 = 17" in hdr and "TSD_MODEL_CONTROLNET_SD15_TORCH = 11" in hdr


def test_parameter_specs_of_the_sd2_unet(tsd_mod):
    s16, s6, s5 = (tsd_mod.param_specs(k) for k in ("diffusion_sd2", "diffusion_sd15_torch", "diffusion_sd15"))
    assert [n for n, *_ in s16] == [n for n, *_ in s6]                      # names and order are kind 6's
    d16, d6 = {n: sh for n, sh, *_ in s16}, {n: sh for n, sh, *_ in s6}
    differ = sorted(n for n in d16 if d16[n] != d6[n])
    assert differ and all(n.endswith(("layer6.k_proj.weight", "layer6.v_proj.weight")) for n in differ)
    blocks = sorted({n.rsplit(".layer4.in_proj.weight", 1)[0] for n in d16 if n.endswith(".layer4.in_proj.weight")})
    assert len(blocks) == 16
    for b in blocks:
        C = d16[b + ".layer4.in_proj.weight"][1]
        assert C in (320, 640, 1280) and d16[b + ".layer4.in_proj.weight"] == (3 * C, C)
        assert d16[b + ".layer6.k_proj.weight"] == (C, 1024) and d16[b + ".layer6.v_proj.weight"] == (C, 1024)
        assert d6[b + ".layer6.k_proj.weight"] == (C, 768)
    n5 = len(s5)                                                            # the norms come last, behind everything kind 5 has
    assert [n for n, *_ in s16[:n5]] == [n for n, *_ in s5]
    assert all(len(sh) == 1 and (n.endswith(".weight") or n.endswith(".bias")) and ".layer" in n or n.startswith("final.layer1") for n, sh, *_ in s16[n5:])
    assert s16[-1][0] == "final.layer1.bias"


def test_parameter_specs_of_the_sd2_text_encoder(tsd_mod):
    s17, s7 = tsd_mod.param_specs("clip_sd2"), tsd_mod.param_specs("clip_torch")
    d = {n: sh for n, sh, *_ in s17}
    assert d["embedding.token.weight"] == (49408, 1024) and d["embedding.position"] == (77 * 1024,)
    assert "player23.layer5.weight" in d and "player24.layer5.weight" not in d and "player13.layer5.weight" not in {n for n, *_ in s7}
    assert d["player1.layer2.in_proj.weight"] == (3072, 1024) and d["player23.layer4.weight"] == (4096, 1024)
    assert d["layernorm.weight"] == (1024,) and s17[-1][0] == "layernorm.bias"
    assert len(s17) == 2 + 23 * 8 + 23 * 4 + 2


def test_flop_count_uses_the_context_width(tsd_mod):
    f16, f6 = tsd_mod.flop_count("diffusion_sd2", 64), tsd_mod.flop_count("diffusion_sd15_torch", 64)
    widths = [sh[0] for n, sh, *_ in tsd_mod.param_specs("diffusion_sd2") if n.endswith("layer6.k_proj.weight")]
    extra = sum(2 * 2.0 * 77 * (1024 - 768) * C for C in widths) / 1e9      # k_proj and v_proj over 256 more context columns
    assert abs((f16 - f6) - extra) < 1e-6 * f16 and extra > 0
    assert tsd_mod.flop_count("clip_sd2", 0) > 3 * tsd_mod.flop_count("clip_torch", 0)


def test_a_wrong_context_width_names_both_widths(tsd_mod):
    msg = tsd_mod.model._context_error("context", (2, 77, 1024), (2, 77, 768))
    assert "1024" in msg and "768" in msg and "wide" in msg
    assert "wide" not in tsd_mod.model._context_error("context", (2, 77, 1024), (1, 77, 1024))


def _small(specs):
    """One small array per parameter, its rank kept: round trips of the key maps need names and ranks, not 865 M floats."""
    g, out = np.random.default_rng(3), {}
    for name, shape, used, _ in specs:
        if not used:
            continue
        s = [2] * len(shape)
        if name.endswith("in_proj.weight") or name.endswith("in_proj.bias"):
            s[0] = 6
        elif len(shape) == 4:
            s = [3 if shape[0] != shape[1] else 2, 2, shape[2], shape[3]]
        if name == "embedding.token.weight":
            s = [4, shape[1]]
        if name == "embedding.position":
            s = [77 * 1024 if shape[0] == 77 * 1024 else 77 * 768]
        out[name] = g.standard_normal(s).astype(np.float32)
    return out


def test_unet_key_map_round_trips_with_proj_in_2d_and_4d(tsd_mod):
    from tsd import checkpoint as ck
    P = _small(tsd_mod.param_specs("diffusion_sd2"))
    for linear in (True, False):
        state = ck.params_to_diffusers_sd2_unet(P, linear_projection=linear)
        proj = [k for k in state if k.endswith(("proj_in.weight", "proj_out.weight"))]
        assert len(proj) == 32 and all(state[k].ndim == (2 if linear else 4) for k in proj)
        assert all(k.split(".")[0] in ("conv_in", "down_blocks", "mid_block", "up_blocks", "time_embedding", "conv_norm_out", "conv_out") for k in state)
        back = ck.diffusers_sd2_unet_to_params(state)
        assert set(back) == set(P) and all(back[k].shape == P[k].shape and np.array_equal(back[k], P[k]) for k in P), linear


def test_text_encoder_key_map_round_trips_and_names_its_variant(tsd_mod):
    from tsd import checkpoint as ck
    for kind, layers in (("clip_sd2", 23), ("clip_torch", 12)):
        P = _small(tsd_mod.param_specs(kind))
        state = ck.params_to_hf_clip_text(P)
        assert f"text_model.encoder.layers.{layers - 1}.mlp.fc2.bias" in state and f"text_model.encoder.layers.{layers}.mlp.fc2.bias" not in state
        back = ck.hf_clip_text_to_params(state)
        assert set(back) == set(P) and all(np.array_equal(back[k].reshape(P[k].shape), P[k]) for k in P)
        assert ck.clip_text_variant(back) == kind
