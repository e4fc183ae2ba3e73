"""GPU: the torch-norm kinds of the fused attention-block kernels - attn_chain_kernel<KIND_HEAD_T> / <KIND_TAIL_T> (csrc/kernels_chain.hip):
GroupNorm / LayerNorm affine, rsqrt(var + eps), exact GELU - held to chain_affine_ref's float64 reference through
tsd_debug_chain_run_affine under chain_ref's limits as they stand, reduced to the plain kernels at the identity affine, and at the
model level (kind 6, TSD_CHAIN = 2) against the op-by-op graph and the numpy restatement.  Run as a program (`jitter-child <repeats>`)
it prints the digests of the replay cases on whatever library TSD_LIB names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "stable-diffusion.mojo_amd"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import chain_affine_ref as A
import chain_ref as R
import jitter_manifest
import replay

pytestmark = pytest.mark.gpu
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
JITTER_REPEATS = 8
# one workgroup and 2 x 128; T = 1, 64 (fragment 4 all masked), 77, 80 (pad keys, fragment 4 full); partials on and off; wide pitches; the two
# input kinds that stress LayerNorm (a mean per column quarter) and the GELU (gates over +-12)
CASES = [(f"tail/S64_T{T}_gn{gn}", R.tail_desc(1, 64, T=T, gn=gn, ldvt=88), "flat") for T, gn in ((1, 0), (64, 1), (77, 0), (80, 1))]
CASES += [(f"tail/B2_S128_{k}", R.tail_desc(2, 128, gn=1), k) for k in ("flat", "ln_offset", "wide_gates")]
CASES += [("tail/B3_S64_pitched", R.tail_desc(3, 64, **R.PITCHED), "flat"),
          ("head/B1_S64", R.head_desc(1, 64), "flat"), ("head/B2_S128", R.head_desc(2, 128), "group_means"),
          ("head/B3_S64_pitched", R.head_desc(3, 64, ld_vt=72, **R.HEAD_PITCHED), "group_means")]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def ctx(gpu_ctx, tsd_mod):
    c = tsd_mod.Context(gpu_ctx.device)
    assert replay.lib().tsd_debug_set_fused_attention(c.h, 2) == 1
    yield c
    c.close()


def inputs(case):
    name, d, kind = case
    return d, R.make_inputs(d, kind, seed=R.SEED), A.draw_affine(IDS.index(name))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_torch_kernel_matches_the_fp64_reference(ctx, case):
    d, ops, aff = inputs(case)
    rc, outs, info = A.run(ctx, d, ops, aff)
    assert rc == 0, replay.lib().tsd_last_error().decode()
    assert info == {"CHANGED": 0, "RAN": 2}, info                     # RAN = 2: the torch-norm kernel
    fails, worst = R.check(d, ops, outs, A.emulate(d, ops, aff), A.reference(d, ops, aff))
    print(f"[chain-affine] {case[0]}: worst ratio to the limit " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not fails, "; ".join(fails)
    again = A.run(ctx, d, ops, aff)[1]
    assert all(np.array_equal(outs[s].view(np.uint8), again[s].view(np.uint8)) for s in outs), "a second run gave other bits"


@pytest.mark.parametrize("case", [CASES[9], CASES[10]], ids=IDS[9:11])
def test_head_at_the_identity_affine_is_the_plain_head_bit_for_bit(ctx, case):
    """gamma = 1, beta = 0 and the reference's rstd: HTOK, QK and HVT - every head output - carry the plain kernel's bits."""
    d, ops, _ = inputs(case)
    rc, got, info = A.run(ctx, d, ops, A.IDENTITY, A.REF_RSTD)
    rc0, want, info0 = replay.run("tsd_debug_chain_run", ctx, d, ops, R.CO, R.INPUTS, R.OUTPUTS, R.dtype_of, R.extents)
    assert rc == 0 and rc0 == 0 and info["RAN"] == 2 and int(info0[R.CI["RAN"]]) == 1
    assert all(np.array_equal(got[s].view(np.uint16), want[s].view(np.uint16)) for s in ("HTOK", "QK", "HVT"))


def test_tail_at_the_identity_affine_differs_from_the_plain_tail_by_the_gelu_only(ctx):
    """No tail output is bitwise: OUT (and its partials) lies behind the GELU.  |y_T - y_0| <= |ref_erf - ref_tanh| + tol_T + tol_0 element-wise,
    tol = ulp16(ref) / 2 + K_ELEM r(row) of chain_ref.check for either kernel."""
    d, ops, _ = inputs(CASES[6])      # wide gates: tanh and erf forms differ most around |g| = 2
    got = A.run(ctx, d, ops, A.IDENTITY, A.REF_RSTD)[1]
    want = replay.run("tsd_debug_chain_run", ctx, d, ops, R.CO, R.INPUTS, R.OUTPUTS, R.dtype_of, R.extents)[1]
    y1, y0 = (R.token_major(d, "OUT", o["OUT"]).astype(np.float64) for o in (got, want))
    r1, r0 = A.reference(d, ops, A.IDENTITY, erf=True, torch=False)["OUT"], R.reference(d, ops)["OUT"]
    e1, e0 = A.emulate(d, ops, A.IDENTITY, erf=True, torch=False)[1]["OUT"], R.emulate(d, ops)[1]["OUT"]
    tol = sum(R.ulp16(r) / 2 + R.K_ELEM * R._rms(e.astype(np.float64) - r, 1)[:, None] for r, e in ((r1, e1), (r0, e0)))
    assert not np.array_equal(y1, y0) and (np.abs(y1 - y0) <= np.abs(r1 - r0) + tol).all()


def test_torch_kernel_needs_switch_2(ctx):
    d, ops, aff = inputs(CASES[0])
    L = replay.lib()
    assert L.tsd_debug_set_fused_attention(ctx.h, 1) == 2
    try:
        rc, outs, info = A.run(ctx, d, ops, aff)
    finally:
        assert L.tsd_debug_set_fused_attention(ctx.h, 2) == 1
    assert rc != 0 and info == {"CHANGED": 0, "RAN": 0}
    replay.assert_untouched(outs, "switch 1")


def model_case(tsd_mod):
    """A seeded kind-6 UNet and a B = 2 forward at 16 x 16 (the jitter comparison needs the same weights in two processes)."""
    import freeu_ref as F
    one = F.model_inputs(KIND, 16, 16)
    return tsd_mod.Diffusion(seed=5, variant=KIND), [np.concatenate([a, np.ascontiguousarray(a[..., ::-1]) * 0.8]) for a in one[:2]] + [np.concatenate([one[2], one[2]])]


def digests(tsd_mod, ctx, repeats):
    out = []
    for case in (CASES[1], CASES[6], CASES[10]):
        d, ops, aff = inputs(case)
        got = [A.run(ctx, d, ops, aff)[1] for _ in range(repeats)]
        out.append((case[0], [jitter_manifest.digest("chain_affine", [g[s] for s in sorted(g)]) for g in got]))
    m, x = model_case(tsd_mod)
    try:
        out.append(("kind6_forward", [jitter_manifest.digest("chain_affine", [at_switch(tsd_mod.default_context(), 2, lambda: m.forward(*x))]) for _ in range(repeats)]))
    finally:
        m.model.close()
    return out


def test_bits_do_not_depend_on_the_run_nor_on_the_jitter_build(ctx, tsd_mod):
    here = digests(tsd_mod, ctx, 3)
    assert all(len(set(d)) == 1 for _, d in here), here
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`)")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [(t["name"], set(t["digests"])) for t in there] == [(n, {dg[0]}) for n, dg in here]


# ---- the models: kind 6 and its ControlNet (torch norms, exact GELU) at 16 x 16 latents - S = 256 at the C = 320 level -, B = 2, T = 77 --------
KIND, CN_KIND = "diffusion_sd15_torch", "controlnet_sd15_torch"


def at_switch(gpu_ctx, v, fn):
    L = replay.lib()
    old = L.tsd_debug_set_fused_attention(gpu_ctx.h, v)
    try:
        return fn()
    finally:
        L.tsd_debug_set_fused_attention(gpu_ctx.h, old)


def chain_launches(gpu_ctx, v, fn):
    """Launches of the fused kernels' class (a head and a tail per C = 320 block) in fn() at switch v, from the per-launch profile."""
    def profiled():
        gpu_ctx.profile_begin()
        try:
            fn()
            return sum(1 for r in gpu_ctx.profile_records() if r[0] == "attn_tail_chain")
        finally:
            gpu_ctx.profile_end()
    return at_switch(gpu_ctx, v, profiled)


@pytest.fixture(scope="module")
def world(gpu_ctx, tsd_mod):
    import controlnet_ref as CR
    import freeu_ref as F
    P, PC = CR.draw_params(tsd_mod.param_specs(KIND), F.MODEL_SEED), CR.draw_params(tsd_mod.param_specs(CN_KIND), 5, nonzero=("zero.", "hint.conv8"))
    one = F.model_inputs(KIND, 16, 16)
    x = [np.concatenate([a, np.ascontiguousarray(a[..., ::-1]) * 0.8]) for a in one[:2]] + [np.concatenate([one[2], one[2]])]
    hint = np.random.default_rng(11).uniform(0, 1, (2, 3, 128, 128)).astype(np.float32)
    ref = np.stack([F.diffusion_freeu(P, x[0][b], x[1][b], x[2][b], None, steps=F.model_steps(KIND), tn=True) for b in range(2)])
    res = [CR.controlnet(PC, x[0][b], x[1][b], x[2][b], hint[b], tn=True) for b in range(2)]
    w = dict(d=tsd_mod.Diffusion(params=P, variant=KIND), cn=tsd_mod.ControlNet(params=PC, variant=CN_KIND), ip=tsd_mod.IPAdapter(seed=9), x=x, hint=hint, ref=ref,
             res=[np.stack([res[b][k] for b in range(2)]) for k in range(13)],
             plain_d=tsd_mod.Diffusion(seed=3, variant="diffusion_sd15"), plain_cn=tsd_mod.ControlNet(seed=3, variant="controlnet_sd15"))
    yield w
    for k in ("d", "cn", "ip", "plain_d", "plain_cn"):
        w[k].model.close()


def test_kind_6_forward_at_switch_2(gpu_ctx, world):
    """Against the op-by-op graph within test_fused_attention_blocks_match_unfused_graph_at_full_size's 3e-3 and against the numpy restatement
    within TOL_MODEL; every C = 320 block leaves the op-by-op path: as many fused launches as the plain kind 5, which has the same step table, and
    none at the default switch, whose bits a visit to 2 leaves alone; a sample's bits do not depend on its place in the batch."""
    from util import TOL_MODEL, rel_l2
    d, x, ref = world["d"], world["x"], world["ref"]
    s1 = d.forward(*x)
    s2 = at_switch(gpu_ctx, 2, lambda: d.forward(*x))
    s0 = at_switch(gpu_ctx, 0, lambda: d.forward(*x))
    third = at_switch(gpu_ctx, 2, lambda: d.forward(*[np.concatenate([a[:1], a[:1], a[1:2]]) for a in x]))
    print(f"[chain-affine] kind 6: switch 2 against 0 {rel_l2(s2, s0):.3e}, against the restatement {rel_l2(s2, ref):.3e} (switch 1: {rel_l2(s1, ref):.3e})")
    assert np.isfinite(s2).all() and rel_l2(s2, s0) < 3e-3 and rel_l2(s2, ref) <= TOL_MODEL
    n_plain = chain_launches(gpu_ctx, 1, lambda: world["plain_d"].forward(*x))
    assert n_plain >= 4 and chain_launches(gpu_ctx, 2, lambda: d.forward(*x)) == n_plain and chain_launches(gpu_ctx, 1, lambda: d.forward(*x)) == 0
    assert np.array_equal(d.forward(*x), s1)
    assert np.array_equal(at_switch(gpu_ctx, 2, lambda: d.forward(*x)), s2) and np.array_equal(third[2], s2[1])


def test_kind_11_residuals_at_switch_2(gpu_ctx, world):
    from util import TOL_MODEL, rel_l2
    cn, x, hint = world["cn"], world["x"], world["hint"]
    fwd = lambda m=cn: m.forward(*x, hint)   # noqa: E731
    r1, r2, r0 = fwd(), at_switch(gpu_ctx, 2, fwd), at_switch(gpu_ctx, 0, fwd)
    for k in range(13):
        assert np.isfinite(r2[k]).all() and rel_l2(r2[k], r0[k]) < 3e-3 and rel_l2(r2[k], world["res"][k]) <= TOL_MODEL, k
    n_plain = chain_launches(gpu_ctx, 1, lambda: fwd(world["plain_cn"]))
    assert n_plain >= 2 and chain_launches(gpu_ctx, 2, fwd) == n_plain and chain_launches(gpu_ctx, 1, fwd) == 0
    assert all(np.array_equal(a, b) for a, b in zip(fwd(), r1)) and not all(np.array_equal(a, b) for a, b in zip(r2, r1))


def test_blocks_that_must_stay_op_by_op_under_switch_2(gpu_ctx, world):
    """An IP-Adapter forward and the FP8 feed-forward: no fused launch, switch 1's bits."""
    d, x, ip = world["d"], world["x"], world["ip"]
    tok = ip.project(np.random.default_rng(12).standard_normal((2, 1024)).astype(np.float32))
    adapted = lambda: d.forward(*x, ip_adapter=ip, ip_tokens=tok, ip_scale=(0.7, 0.4))   # noqa: E731
    assert np.array_equal(at_switch(gpu_ctx, 2, adapted), adapted()) and chain_launches(gpu_ctx, 2, adapted) == 0
    d.set_ff_fp8(True)
    try:
        assert np.array_equal(at_switch(gpu_ctx, 2, lambda: d.forward(*x)), d.forward(*x))
    finally:
        d.set_ff_fp8(False)


def test_kind_5_does_not_see_the_switch_value(gpu_ctx, world):
    d, x = world["plain_d"], world["x"]
    assert np.array_equal(at_switch(gpu_ctx, 2, lambda: d.forward(*x)), d.forward(*x))


def test_kind_16_does_not_see_the_switch_value(gpu_ctx, tsd_mod):
    import freeu_ref as F
    d, x = tsd_mod.Diffusion(seed=3, variant="diffusion_sd2"), F.model_inputs("diffusion_sd2", 16, 16)
    try:
        assert np.array_equal(at_switch(gpu_ctx, 2, lambda: d.forward(*x)), d.forward(*x))
    finally:
        d.model.close()


def test_cfg_session_at_switch_2_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod):
    import test_gpu_controlnet as TC   # the host-driven loop and the session driver
    case, inp = TC.S_CASES[0], TC._s_inputs(2300)   # seeded DDPM
    d = tsd_mod.Diffusion(seed=TC.SEED, variant=KIND)
    try:
        with TC.hoist(tsd_mod, gpu_ctx, 1):
            plain = TC.session_run(tsd_mod, d, None, case, True, inp, None)
            got = at_switch(gpu_ctx, 2, lambda: TC.session_run(tsd_mod, d, None, case, True, inp, None))
            want = at_switch(gpu_ctx, 2, lambda: TC.host_loop(tsd_mod, gpu_ctx, d, None, case, True, inp, lambda i: None))
    finally:
        d.model.close()
    assert all(np.isfinite(g).all() and TC._same(g, w) for g, w in zip(got, want)) and not TC._same(got[-1], plain[-1])


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    import tsd
    tsd.set_strict(True)
    _c = tsd.Context(0)
    replay.lib().tsd_debug_set_fused_attention(_c.h, 2)
    for _name, _digests in digests(tsd, _c, int(sys.argv[2])):
        print(json.dumps({"name": _name, "digests": _digests}), flush=True)
