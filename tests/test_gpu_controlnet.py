"""GPU: ControlNet on the full-size UNet - the injection kernel alone (tsd.control_inject) against its exact fp64 statement, the 13
residuals of both ControlNet kinds and the controlled UNet forward against the numpy restatement (tests/controlnet_ref.py), the
statistics hand-over, the diffusers import, the refusals, and the -DTSD_JITTER build held to the shipped bits.

The zero convolutions and the hint encoder's last layer are drawn with bound 1 / sqrt(fan_in): at their zero initialisation every
residual is zero and every test here would pass without the feature.

Measured on an MI355X: residuals 4.6e-4 ... 1.9e-3 relative L2 (growing with depth), controlled forward 1.3e-3 - 1.4e-3, control against no
control 0.50 - 0.53, injection partials at most 1 % of their bound.  Statistics hand-over (L = 16, B = 2, scales (1, 0.5)): the controlled
forward with the injection's statistics and the one whose consumers recompute them are NOT bitwise equal - DESIGN.md 4.14 says why - so
both are held to the reference and their difference to the split-K yardstick: reference kind 1.016e-3 between the routes against 1.077e-3
between split-K on and off, torch kind 1.070e-3 against 1.095e-3; 1.35e-3 / 1.32e-3 and 1.36e-3 to the reference.  That yardstick is the
whole forward under another launch plan of the same layers (tile choices other than split-K are bitwise equal here), the margin is 2 - 6 %,
and at L = 16 only the 256- and 64-pixel levels carry producer statistics (one slab per 32 rows: none at 16 and 4 pixels), so the in-graph
hand-over is exercised on 7 of the 13 tensors; the 16- and 4-pixel geometries are held by the kernel test's table.  Sessions (group 4):
bitwise the host-driven loops in all 12 sampler x CFG x hoist cases.  The whole file: 28 s.

Run as `python tests/test_gpu_controlnet.py jitter-child REPEATS` this file is the child of the jitter test: it prints one JSON line of
digests per case on whatever library TSD_LIB names."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "stable-diffusion.mojo_amd"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import pytest

import controlnet_ref as R
from oracle import ops, rng, spec
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, rel_l2

pytestmark = pytest.mark.gpu
SEED = 1234
CN_SEED = 5
T = 77
VARIANTS = {"reference": ("controlnet_sd15", "diffusion_sd15", False), "torch": ("controlnet_sd15_torch", "diffusion_sd15_torch", True)}
SHAPES = ((16, 16), (16, 32))
SCALES = (1.0, 0.5)
NONZERO = ("zero.", "hint.conv8")
JITTER_REPEATS = 8
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")

# ---- 1. the injection kernel ------------------------------------------------------------------------------------------------------------
# (HW, C, groups, nslab): three levels of the UNet, a slab shorter than 32 rows with the fine groups of concat_stat_groups, and one entry
# without statistics
TABLE = ((256, 320, 32, 8), (64, 640, 32, 2), (16, 1280, 32, 1), (4, 1280, 64, 1), (48, 320, 0, 2))
TABLE_B = 3
TABLE_SCALES = np.array([0.0, 1.0, 0.37], np.float32)


def _f16_exact(g, shape):
    """fp16 values with magnitudes in [2^-6, 2^6) or exactly 0: s * r + x is then exact in fp64 for an fp32 s."""
    e = g.integers(-6, 6, size=shape)
    m = g.integers(0, 1024, size=shape)
    v = np.ldexp(1.0 + m / 1024.0, e) * g.choice([-1.0, 1.0], size=shape)
    v[g.random(shape) < 0.1] = 0.0
    out = v.astype(np.float16)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def inject_table():
    g = np.random.default_rng(11)
    xs = [_f16_exact(g, (TABLE_B, hw, c)) for hw, c, _, _ in TABLE]
    rs = [_f16_exact(g, (TABLE_B, hw, c)) for hw, c, _, _ in TABLE]
    return xs, rs, [q[2] for q in TABLE], [q[3] for q in TABLE]


def _digest(arrays):
    h = hashlib.sha1()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_injection_kernel_is_the_exact_fma_and_emits_the_statistics_of_what_it_wrote(gpu_ctx, tsd_mod):
    xs, rs, groups, nslab = inject_table()
    ys, ps = tsd_mod.control_inject(xs, rs, TABLE_SCALES, groups, nslab)
    s64 = TABLE_SCALES.astype(np.float64)[:, None, None]
    for (hw, c, G, ns), x, r, y, p in zip(TABLE, xs, rs, ys, ps):
        want = (s64 * r.astype(np.float64) + x.astype(np.float64)).astype(np.float32).astype(np.float16)
        assert np.array_equal(want.view(np.uint16), y.view(np.uint16)), f"{(hw, c)}: y is not f16(f32(f64(s) * r + x)) bitwise"
        assert np.array_equal(y[0], x[0]), f"{(hw, c)}: y != x at s = 0"
        if not G:
            assert p is None
            continue
        sp = -(-hw // ns)
        yy = y.astype(np.float64).reshape(TABLE_B, ns, sp, G, c // G)
        n = sp * (c // G)
        e1 = np.abs(p[..., 0] - yy.sum((2, 4)))
        e2 = np.abs(p[..., 1] - (yy * yy).sum((2, 4)))
        b1, b2 = n * 2.0 ** -24 * np.abs(yy).sum((2, 4)), n * 2.0 ** -24 * (yy * yy).sum((2, 4))
        print(f"[inject] {(hw, c, G, ns)}: n={n} sum err {e1.max():.3e} (bound >= {b1.min():.3e}) squares err {e2.max():.3e} (bound >= {b2.min():.3e})")
        assert (e1 <= b1).all() and (e2 <= b2).all(), f"{(hw, c, G, ns)}: partials outside n 2^-24 sum|y| / sum y^2"
    again = tsd_mod.control_inject(xs, rs, TABLE_SCALES, groups, nslab)
    assert _digest(ys + ps) == _digest(again[0] + again[1]), "two runs differ"
    perm = [2, 0, 1]  # a sample's y and partials do not depend on its batch position
    ym, pm = tsd_mod.control_inject([x[perm] for x in xs], [r[perm] for r in rs], TABLE_SCALES[perm], groups, nslab)
    for y, p, y2, p2 in zip(ys, ps, ym, pm):
        assert np.array_equal(y[perm].view(np.uint16), y2.view(np.uint16))
        assert p is None or np.array_equal(p[perm], p2)


def test_injection_entry_refusals(gpu_ctx, tsd_mod):
    x = np.zeros((1, 8, 16), np.float16)
    for bad, kw in ((tsd_mod._lib.TSD_E_SHAPE, dict(groups=[3], nslab=[1])),      # 16 channels in 3 groups
                    (tsd_mod._lib.TSD_E_SHAPE, dict(groups=[2], nslab=[9])),      # more slabs than rows
                    (tsd_mod._lib.TSD_E_SHAPE, dict(groups=[2], nslab=[5]))):     # ceil(8 / 5) * 4 >= 8: an empty last slab
        with pytest.raises(tsd_mod.TsdError) as e:
            tsd_mod.control_inject([x], [x], [1.0], **kw)
        assert e.value.code == bad
    with pytest.raises(tsd_mod.TsdError) as e:
        tsd_mod.control_inject([np.zeros((1, 8, 12), np.float16)] * 1, [np.zeros((1, 8, 12), np.float16)], [1.0], [0], [1])  # C % 8
    assert e.value.code == tsd_mod._lib.TSD_E_SHAPE


# ---- 2 - 5. the models ------------------------------------------------------------------------------------------------------------------
def _inputs(B, LH, LW, tag):
    lat = rng.normal(7, tag, B * 4 * LH * LW).reshape(B, 4, LH, LW)
    ctx = rng.normal(7, tag + 1, B * T * 768).reshape(B, T, 768)
    hint = (rng.uniform(7, tag + 2, B * 3 * 64 * LH * LW, 0.5) + np.float32(0.5)).reshape(B, 3, 8 * LH, 8 * LW)  # an image in [0, 1]
    temb = np.stack([ops.time_embedding(t) for t in (980.0, 20.0, 500.0)[:B]])
    return lat, ctx, temb, hint


class World:
    """Both models of one variant, built once per module, with the reference of every shape computed once and kept unchanged."""

    def __init__(self, tsd_mod, name):
        self.name = name
        self.cn_kind, self.unet_kind, self.tn = VARIANTS[name]
        self.PC = R.draw_params(tsd_mod.param_specs(self.cn_kind), CN_SEED, nonzero=NONZERO)
        self.cn = tsd_mod.ControlNet(params=self.PC, variant=self.cn_kind)
        self.d = tsd_mod.Diffusion(seed=SEED, variant=self.unet_kind)
        PU = spec.init_params(self.unet_kind, SEED, only_used=not self.tn)
        self.cases = {}
        for i, (LH, LW) in enumerate(SHAPES):
            lat, ctx, temb, hint = _inputs(2, LH, LW, 700 + 10 * i)
            res = [R.controlnet(self.PC, lat[b], ctx[b], temb[b], hint[b], tn=self.tn) for b in range(2)]
            ref = np.stack([R.diffusion_sd15_controlled(PU, lat[b], ctx[b], temb[b], res[b], SCALES[b], tn=self.tn) for b in range(2)])
            self.cases[(LH, LW)] = dict(lat=lat, ctx=ctx, temb=temb, hint=hint, res=[np.stack([res[b][k] for b in range(2)]) for k in range(13)],
                                        ref=ref)
        del PU
        self._out = {}

    def controlled(self, shape, scale=SCALES):
        """The controlled forward of `shape`; the one at SCALES is computed once and shared."""
        c = self.cases[shape]
        if scale is SCALES and shape in self._out:
            return self._out[shape]
        out = self.d.forward(c["lat"], c["ctx"], c["temb"], control=self.cn, hint=c["hint"], control_scale=scale)
        if scale is SCALES:
            self._out[shape] = out
        return out

    def close(self):
        self.cn.model.close()
        self.d.model.close()


@pytest.fixture(scope="module", params=list(VARIANTS))
def world(request, gpu_ctx, tsd_mod):
    w = World(tsd_mod, request.param)
    yield w
    w.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_residuals_match_the_reference(world, shape):
    c = world.cases[shape]
    got = world.cn.forward(c["lat"], c["ctx"], c["temb"], c["hint"])
    assert len(got) == 13
    for k in range(13):
        assert np.abs(c["res"][k]).max() > 0.1   # the zero convolutions are not at zero here
        assert_close(got[k], c["res"][k], TOL_MODEL, TOL_MODEL_MAX, f"{world.name} {shape} residual {k}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_controlled_forward_matches_the_reference_and_scale_zero_is_the_plain_forward(world, shape):
    c = world.cases[shape]
    out = world.controlled(shape)
    assert_close(out, c["ref"], TOL_MODEL, TOL_MODEL_MAX, f"{world.name} {shape} controlled forward")
    plain = world.d.forward(c["lat"], c["ctx"], c["temb"])
    acts = rel_l2(out, plain)
    print(f"[control] {world.name} {shape}: rel_l2 against the uncontrolled forward {acts:.3e}")
    assert acts > 10 * TOL_MODEL, "the control does not act on these weights"
    np.testing.assert_array_equal(world.d.forward(c["lat"], c["ctx"], c["temb"], control=world.cn, hint=c["hint"], control_scale=SCALES), out)
    np.testing.assert_array_equal(world.controlled(shape, scale=0.0), plain)
    # per-sample scales: sample 1 at scale 0 is sample 1 of the plain forward, sample 0 at scale 1 is sample 0 of the controlled one
    mixed = world.controlled(shape, scale=(1.0, 0.0))
    np.testing.assert_array_equal(mixed[1], plain[1])
    np.testing.assert_array_equal(mixed[0], out[0])


def test_statistics_hand_over(world, tsd_mod, gpu_ctx):
    """The injection's statistics against every consumer recomputing them (TSD_CONTROL_STATS = 0).  The two are not bitwise equal
    (the consumers' own pass sums other slabs in another order), so both are held to the reference and their difference
    below the one between two launch plans of the same layers: split-K on (the default) and off (TSD_GEMM_SPLITK = 0)."""
    shape = SHAPES[0]
    c = world.cases[shape]
    out = world.controlled(shape)
    lib = tsd_mod._lib.lib()
    prev = lib.tsd_debug_set_control_stats(gpu_ctx.h, 0)
    try:
        recomputed = world.d.forward(c["lat"], c["ctx"], c["temb"], control=world.cn, hint=c["hint"], control_scale=SCALES)
    finally:
        lib.tsd_debug_set_control_stats(gpu_ctx.h, prev)
    assert prev == 1
    assert_close(out, c["ref"], TOL_MODEL, TOL_MODEL_MAX, f"{world.name} with the injection's statistics")
    assert_close(recomputed, c["ref"], TOL_MODEL, TOL_MODEL_MAX, f"{world.name} with recomputed statistics")
    os.environ["TSD_GEMM_SPLITK"] = "0"
    try:
        ctx2 = tsd_mod.Context(gpu_ctx.device)
    finally:
        del os.environ["TSD_GEMM_SPLITK"]
    cn2 = tsd_mod.ControlNet(params=world.PC, variant=world.cn_kind, ctx=ctx2)
    d2 = tsd_mod.Diffusion(seed=SEED, variant=world.unet_kind, ctx=ctx2)
    try:
        unsplit = d2.forward(c["lat"], c["ctx"], c["temb"], control=cn2, hint=c["hint"], control_scale=SCALES)
    finally:
        cn2.model.close(); d2.model.close(); ctx2.close()
    hand_over, yardstick = rel_l2(recomputed, out), rel_l2(unsplit, out)
    print(f"[control] {world.name}: bitwise {np.array_equal(recomputed, out)}; statistics paths differ by {hand_over:.3e}, split-K on / off by {yardstick:.3e}")
    assert hand_over <= yardstick


def test_import_through_the_diffusers_key_map(tsd_mod, gpu_ctx):
    """A ControlNet built from what a diffusers ControlNetModel file would hold equals the directly initialised one bit for bit."""
    from tsd import checkpoint as ck
    P = R.draw_params(tsd_mod.param_specs("controlnet_sd15_torch"), CN_SEED, nonzero=NONZERO)
    direct = tsd_mod.ControlNet(params=P, variant="controlnet_sd15_torch")
    other = ck.load_controlnet(ck.params_to_diffusers_controlnet(P))
    lat, ctx, temb, hint = _inputs(2, 16, 16, 700)
    try:
        a, b = direct.forward(lat, ctx, temb, hint), other.forward(lat, ctx, temb, hint)
    finally:
        direct.model.close(); other.model.close()
    for k in range(13):
        assert np.abs(a[k]).max() > 0.1
        np.testing.assert_array_equal(a[k], b[k])


def test_refusals(world, tsd_mod, gpu_ctx):
    E = tsd_mod._lib
    c = world.cases[SHAPES[0]]
    tiny = tsd_mod.Diffusion(seed=SEED)
    ctx2 = tsd_mod.Context(gpu_ctx.device)
    far = tsd_mod.ControlNet(seed=1, variant=world.cn_kind, ctx=ctx2)
    try:
        with pytest.raises(tsd_mod.TsdError) as e:   # the Tiny-SD graph has no ControlNet
            tiny.forward(c["lat"], c["ctx"], c["temb"], control=world.cn, hint=c["hint"])
        assert e.value.code == E.TSD_E_ARG
        with pytest.raises(tsd_mod.TsdError) as e:   # a `cn` that is no ControlNet
            world.d.forward(c["lat"], c["ctx"], c["temb"], control=world.d, hint=c["hint"])
        assert e.value.code == E.TSD_E_ARG
        with pytest.raises(tsd_mod.TsdError) as e:   # the two models on different contexts
            world.d.forward(c["lat"], c["ctx"], c["temb"], control=far, hint=c["hint"])
        assert e.value.code == E.TSD_E_ARG and "context" in str(e.value)
        with pytest.raises(tsd_mod.TsdError) as e:   # a scale that is not finite
            world.d.forward(c["lat"], c["ctx"], c["temb"], control=world.cn, hint=c["hint"], control_scale=float("nan"))
        assert e.value.code == E.TSD_E_ARG
        with pytest.raises(ValueError):              # a hint of the wrong shape
            world.d.forward(c["lat"], c["ctx"], c["temb"], control=world.cn, hint=c["hint"][:, :, :-8])
        with pytest.raises(tsd_mod.TsdError) as e:   # LoRA on a ControlNet is out of scope
            world.cn.model.lora_add("zero.mid.kernel", np.zeros((1280, 1), np.float32), np.zeros((1, 1280), np.float32), 1.0)
        assert e.value.code == E.TSD_E_ARG
        with pytest.raises(tsd_mod.TsdError) as e:   # a ControlNet is no Diffusion
            tsd_mod._lib.check(E.lib().tsd_diffusion_forward_hw(world.cn.model.h, E.ptr(c["lat"]), E.ptr(c["ctx"]), E.ptr(c["temb"]), 2, 16, 16, T,
                                                                E.ptr(np.empty_like(c["lat"]))))
        assert e.value.code == E.TSD_E_ARG
    finally:
        tiny.model.close(); far.model.close(); ctx2.close()
    assert tsd_mod.flop_count(world.cn_kind, 64) == -1.0


# ---- 4. the session ---------------------------------------------------------------------------------------------------------------------
# L = 16, B = 1, 3 steps.  The host loop makes the session's own launches: ONE forward at the UNet's batch (the latents twice under CFG,
# cond and uncond context, the hint twice, the per-sample scales), then the existing update entries.
import ctypes as C
import contextlib

S_L, S_B, S_STEPS, S_NTRAIN, S_SCALE, S_CFG_SCALE = 16, 1, 3, 1000, 0.8, 7.5
S_KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}
S_SPACINGS = {"leading": 0, "trailing": 1}
# (name, prediction, zero_terminal_snr, (sampler, eta, spacing), noise): DDPM seeded, DPM-Solver++(2M), v-prediction
S_CASES = [("ddpm_seeded", "epsilon", False, ("ddpm", 0.0, "leading"), "seeded"), ("dpmpp_2m", "epsilon", False, ("dpmpp_2m", 0.0, "trailing"), None),
           ("vpred", "v", True, ("ddpm", 0.0, "trailing"), "upload")]
S_SEEDS = [777]


@contextlib.contextmanager
def hoist(tsd_mod, gpu_ctx, on):
    lib = tsd_mod._lib.lib()
    prev = lib.tsd_debug_set_session_hoist(gpu_ctx.h, int(on))
    try:
        yield
    finally:
        lib.tsd_debug_set_session_hoist(gpu_ctx.h, prev)


@pytest.fixture(scope="module")
def pair(gpu_ctx, tsd_mod):
    """The reference-kind UNet and ControlNet for the session tests (no numpy reference: everything is held to the device's own forward)."""
    cn_kind, unet_kind, _ = VARIANTS["reference"]
    cn = tsd_mod.ControlNet(params=R.draw_params(tsd_mod.param_specs(cn_kind), CN_SEED, nonzero=NONZERO), variant=cn_kind)
    d = tsd_mod.Diffusion(seed=SEED, variant=unet_kind)
    yield d, cn
    cn.model.close(); d.model.close()


def _s_inputs(tag):
    lat, ctx, _, hint = _inputs(S_B, S_L, S_L, tag)
    uctx = rng.normal(7, tag + 5, S_B * T * 768).reshape(S_B, T, 768)
    nz = rng.normal(7, tag + 6, S_STEPS * lat.size).reshape((S_STEPS,) + lat.shape)
    return lat, ctx, uctx, hint, nz


def _coeffs(tsd_mod, sampler, i, have_history, pred, ztsnr):
    kind, eta, spacing = sampler
    out = (C.c_double * 8)()
    rc = tsd_mod._lib.lib().tsd_sampler_coeffs_ex(S_KINDS[kind], float(eta), S_SPACINGS[spacing], S_NTRAIN, S_STEPS, 0, i, int(have_history),
                                                  tsd_mod._lib.PREDICTION_TYPES[pred], int(ztsnr), out)
    assert rc == 0, tsd_mod._lib.last_error()
    return np.array(out[:], dtype=np.float64)


def _eps_step(tsd_mod, gpu_ctx, x, e_c, e_u, scale, hist, noise, c, keep_hist):
    from tsd._lib import check, f32, ptr
    x, e_c = f32(x), f32(e_c)
    e_u = f32(e_u) if e_u is not None else None
    out, h = np.empty_like(x), (np.empty_like(x) if keep_hist else None)
    check(tsd_mod._lib.lib().tsd_sampler_step_f32(gpu_ctx.h, ptr(x), ptr(e_c), ptr(e_u), float(scale), ptr(f32(hist)) if hist is not None else None,
                                                  ptr(f32(noise)) if noise is not None else None, x.size, ptr(np.ascontiguousarray(c, dtype=np.float32)),
                                                  ptr(out), ptr(h)))
    return out, h


def _open(tsd_mod, d, cfg, pred, ztsnr, sampler):
    s = tsd_mod.Session(d.model, None, S_B, S_L, T, cfg=cfg)
    s.set_prediction(pred, ztsnr)
    s.set_sampler(*sampler)
    s.set_schedule(S_NTRAIN, S_STEPS, 0)
    return s


def host_forward(tsd_mod, d, cn, x, ctx, uctx, hint, t, scales):
    """The step's forward from the host at the UNet's batch: -> (cond, uncond or None).  scales None: no control."""
    cfg = uctx is not None
    xx = np.concatenate([x, x]) if cfg else x
    cc = np.concatenate([ctx, uctx]) if cfg else ctx
    temb = np.repeat(tsd_mod.get_time_embedding(float(t)).reshape(1, 320), xx.shape[0], axis=0)
    if scales is None:
        e = d.forward(xx, cc, temb)
    else:
        e = d.forward(xx, cc, temb, control=cn, hint=np.concatenate([hint, hint]) if cfg else hint, control_scale=scales)
    return (e[:S_B], e[S_B:]) if cfg else (e, None)


def host_loop(tsd_mod, gpu_ctx, d, cn, case, cfg, inputs, scales_of_step, x0=None, first=0, steps=S_STEPS, extras=None):
    """[latents after step i] of the host-driven loop; scales_of_step(i) -> the per-sample scales of the UNet's batch, or None."""
    _, pred, ztsnr, sampler, noise_kind = case
    lat, ctx, uctx, hint, nz = inputs
    kind = sampler[0]
    x, hist, outs = (lat if x0 is None else x0), None, []
    multistep = kind == "dpmpp_2m"
    for i in range(first, steps):
        cd = _coeffs(tsd_mod, sampler, i, hist is not None, pred, ztsnr)
        e_c, e_u = host_forward(tsd_mod, d, cn, x, ctx, uctx if cfg else None, hint, int(cd[0]), scales_of_step(i))
        if extras and extras.get("phi"):
            e_c, e_u, _ = tsd_mod.cfg_rescale(e_c, e_u, S_CFG_SCALE, extras["phi"], ctx=gpu_ctx)
        if noise_kind == "seeded":
            noise = np.stack([tsd_mod.normal_fill(sd, 16 + i, lat[0].size, ctx=gpu_ctx).reshape(lat[0].shape) for sd in S_SEEDS])
        else:
            noise = nz[i] if noise_kind == "upload" else None
        c = cd[2:].astype(np.float32)
        if pred == "v":
            x, h = tsd_mod.sampler_step_v(x, e_c, e_u, S_CFG_SCALE, hist, noise if (noise is not None and c[5] != 0) else None, c, multistep, ctx=gpu_ctx)
        elif kind == "ddpm":
            x, h = tsd_mod.ddpm_step(x, e_c, e_u, S_CFG_SCALE, noise, i, S_STEPS, S_NTRAIN, 0, sampler[2], ctx=gpu_ctx), None
        else:
            x, h = _eps_step(tsd_mod, gpu_ctx, x, e_c, e_u, S_CFG_SCALE, hist, noise if c[5] != 0 else None, c, multistep)
        hist = h if multistep else None
        if extras and extras.get("mask") is not None:   # the blend of a step with inpainting: the known region at the timestep the update reached
            nxt = _coeffs(tsd_mod, sampler, i + 1, False, pred, ztsnr) if i + 1 < S_STEPS else None
            a_prev, s_prev = (np.float32(nxt[2]), np.float32(nxt[3])) if nxt is not None else (np.float32(1.0), np.float32(0.0))
            x = tsd_mod.inpaint_blend(x, extras["mask"], extras["known"], extras["ip_noise"], a_prev, s_prev, ctx=gpu_ctx)
        outs.append(x)
    return outs


def session_run(tsd_mod, d, cn, case, cfg, inputs, control, extras=None):
    """[latents after step i] of a session; control: None, or the keywords of set_control."""
    _, pred, ztsnr, sampler, noise_kind = case
    lat, ctx, uctx, hint, nz = inputs
    s = _open(tsd_mod, d, cfg, pred, ztsnr, sampler)
    s.upload(lat, ctx, uctx if cfg else None, nz if noise_kind == "upload" else None, cfg_scale=S_CFG_SCALE)
    if noise_kind == "seeded":
        s.set_seeds(S_SEEDS)
    if extras and extras.get("mask") is not None:
        s.set_inpaint(extras["mask"], extras["known"], extras["ip_noise"])
    if extras and extras.get("phi"):
        s.set_guidance_rescale(extras["phi"])
    if control is not None:
        s.set_control(cn, hint, **control)
        assert s.control_active
    outs = []
    for i in range(S_STEPS):
        s.step(i)
        outs.append(s.latents())
    s.close()
    return outs


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("on", [1, 0], ids=["hoist", "nohoist"])
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("case", S_CASES, ids=[c[0] for c in S_CASES])
def test_session_with_control_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, pair, case, cfg, on):
    d, cn = pair
    inputs = _s_inputs(900)
    nb = 2 * S_B if cfg else S_B
    with hoist(tsd_mod, gpu_ctx, on):
        got = session_run(tsd_mod, d, cn, case, cfg, inputs, dict(scale=S_SCALE))
        plain = session_run(tsd_mod, d, cn, case, cfg, inputs, None)
    want = host_loop(tsd_mod, gpu_ctx, d, cn, case, cfg, inputs, lambda i: [S_SCALE] * nb)
    for i in range(S_STEPS):
        assert np.isfinite(got[i]).all()
        assert _same(got[i], want[i]), (case[0], cfg, on, i, float(np.abs(got[i] - want[i]).max()))
    assert rel_l2(got[-1], plain[-1]) > 1e-3   # the control acts on the session's latents


def test_session_cond_only_window_and_turning_control_off(gpu_ctx, tsd_mod, pair):
    d, cn = pair
    case, inputs = S_CASES[0], _s_inputs(910)
    # cond_only: the loop with scales (s, 0)
    got = session_run(tsd_mod, d, cn, case, True, inputs, dict(scale=S_SCALE, cond_only=True))
    want = host_loop(tsd_mod, gpu_ctx, d, cn, case, True, inputs, lambda i: [S_SCALE] * S_B + [0.0] * S_B)
    both = session_run(tsd_mod, d, cn, case, True, inputs, dict(scale=S_SCALE))
    assert all(_same(g, w) for g, w in zip(got, want)) and not _same(got[-1], both[-1])
    # a window first_step = last_step = 1: step 0 is an uncontrolled session's, step 1 the controlled loop's, step 2 the step of an
    # uncontrolled session started from the same state
    win = session_run(tsd_mod, d, cn, case, True, inputs, dict(scale=S_SCALE, first_step=1, last_step=1))
    plain = session_run(tsd_mod, d, cn, case, True, inputs, None)
    assert _same(win[0], plain[0])
    nb = 2 * S_B
    mid = host_loop(tsd_mod, gpu_ctx, d, cn, case, True, inputs, lambda i: [S_SCALE] * nb, x0=win[0], first=1, steps=2)
    assert _same(win[1], mid[0]) and not _same(win[1], plain[1])
    s = _open(tsd_mod, d, True, case[1], case[2], case[3])   # an uncontrolled session started from the state after step 1
    s.upload(win[1], inputs[1], inputs[2], None, cfg_scale=S_CFG_SCALE)
    s.set_seeds(S_SEEDS)
    s.step(2)
    assert _same(win[2], s.latents())
    # set_control(None) restores the uncontrolled bits, on the same session and across an upload()
    s.upload(inputs[0], inputs[1], inputs[2], None, cfg_scale=S_CFG_SCALE)
    s.set_seeds(S_SEEDS)
    s.set_control(cn, inputs[3], scale=S_SCALE)
    s.step(0)
    assert _same(s.latents(), both[0])
    s.upload(inputs[0], inputs[1], inputs[2], None, cfg_scale=S_CFG_SCALE)   # the control outlives the upload
    s.set_seeds(S_SEEDS)
    assert s.control_active
    s.step(0)
    assert _same(s.latents(), both[0])
    s.set_control(None)
    assert not s.control_active
    s.upload(inputs[0], inputs[1], inputs[2], None, cfg_scale=S_CFG_SCALE)
    s.set_seeds(S_SEEDS)
    for i in range(S_STEPS):
        s.step(i)
        assert _same(s.latents(), plain[i])
    s.close()


def test_session_inpainting_guidance_rescale_and_control_in_one_run(gpu_ctx, tsd_mod, pair):
    d, cn = pair
    case = ("ddpm_upload", "epsilon", False, ("ddpm", 0.0, "leading"), "upload")
    inputs = _s_inputs(920)
    cell = np.arange(S_L * S_L).reshape(1, S_L, S_L)
    mask = np.where(cell % 13 < 4, 0.0, np.where(cell % 13 > 9, 1.0, (cell % 13) / 16.0)).astype(np.float32)
    extras = dict(mask=mask, known=rng.normal(7, 925, inputs[0].size).reshape(inputs[0].shape), ip_noise=rng.normal(7, 926, inputs[0].size).reshape(inputs[0].shape),
                  phi=0.7)
    got = session_run(tsd_mod, d, cn, case, True, inputs, dict(scale=S_SCALE), extras)
    want = host_loop(tsd_mod, gpu_ctx, d, cn, case, True, inputs, lambda i: [S_SCALE] * 2, extras=extras)
    for i in range(S_STEPS):
        assert _same(got[i], want[i]), (i, float(np.abs(got[i] - want[i]).max()))
    bare = session_run(tsd_mod, d, cn, case, True, inputs, None, extras)
    assert not _same(got[-1], bare[-1])


def test_session_control_refusals_and_hint_entry(gpu_ctx, tsd_mod, pair):
    d, cn = pair
    E = tsd_mod._lib
    lat, ctx, uctx, hint, _ = _s_inputs(930)
    s = tsd_mod.Session(d.model, None, S_B, S_L, T, cfg=False)
    s.set_schedule(S_NTRAIN, S_STEPS, 0)
    with pytest.raises(tsd_mod.TsdError) as e:       # before upload()
        s.set_control(cn, hint)
    assert e.value.code == E.TSD_E_STATE
    s.upload(lat, ctx, None, None)
    with pytest.raises(tsd_mod.TsdError) as e:       # a `cn` that is no ControlNet
        s.set_control(d, hint)
    assert e.value.code == E.TSD_E_ARG
    with pytest.raises(ValueError):                  # a hint of the wrong shape (the C entry takes no shape: the wrapper owns the check)
        s.set_control(cn, hint[:, :, :-8])
    with pytest.raises(tsd_mod.TsdError) as e:       # a scale that is not finite
        s.set_control(cn, hint, scale=float("inf"))
    assert e.value.code == E.TSD_E_ARG
    ctx2 = tsd_mod.Context(gpu_ctx.device)
    far = tsd_mod.ControlNet(seed=1, ctx=ctx2)
    with pytest.raises(tsd_mod.TsdError) as e:       # another context
        s.set_control(far, hint)
    assert e.value.code == E.TSD_E_ARG
    far.model.close(); ctx2.close()
    assert not s.control_active
    s.set_control(cn, hint)
    with pytest.raises(tsd_mod.TsdError) as e:       # slots_open on a session with control
        s.slots_open()
    assert e.value.code == E.TSD_E_STATE
    s.set_control(None)
    s.slots_open()
    with pytest.raises(tsd_mod.TsdError) as e:       # set_control on a slot session
        s.set_control(cn, hint)
    assert e.value.code == E.TSD_E_STATE
    s.close()
    tiny = tsd_mod.Diffusion(seed=SEED)
    t = tsd_mod.Session(tiny.model, None, S_B, S_L, T, cfg=False)
    t.set_schedule(S_NTRAIN, S_STEPS, 0)
    t.upload(lat, ctx, None, None)
    with pytest.raises(tsd_mod.TsdError) as e:       # the Tiny-SD graph has no ControlNet
        t.set_control(cn, hint)
    assert e.value.code == E.TSD_E_ARG
    t.close(); tiny.model.close()
    # the hint encoder depends on the hint alone: batch position and the other sample do not matter, two runs agree
    h2 = np.concatenate([hint, hint[:, :, ::-1]])
    f2 = cn.hint(h2)
    assert f2.shape == (2, 320, S_L, S_L) and np.isfinite(f2).all() and f2.any() and not np.array_equal(f2[0], f2[1])
    np.testing.assert_array_equal(f2[0], cn.hint(hint[0]))
    np.testing.assert_array_equal(f2, cn.hint(h2))
    with pytest.raises(ValueError):
        tsd_mod.generate_stream(d, None, [], 1, S_L, controlnet=cn, control_image=hint).__next__()


def test_generate_with_a_controlnet_is_the_session_loop(gpu_ctx, tsd_mod, pair):
    d, cn = pair
    lat, ctx, uctx, hint, _ = _s_inputs(940)
    kw = dict(uncond_context=uctx, cfg=True, cfg_scale=S_CFG_SCALE, inference_steps=4, strength=1.0, L=S_L, return_latents=True, seeds=S_SEEDS)
    out = tsd_mod.generate(d, None, ctx, controlnet=cn, control_image=hint, control_scale=S_SCALE, control_start=0.25, control_end=0.75, **kw)
    s = tsd_mod.Session(d.model, None, S_B, S_L, T, cfg=True)
    s.set_schedule(S_NTRAIN, 4, 0)
    s.upload(np.zeros_like(lat), ctx, uctx, None, cfg_scale=S_CFG_SCALE)
    s.set_seeds(S_SEEDS)
    s.seed_latents()
    s.set_control(cn, hint, scale=S_SCALE, first_step=1, last_step=2)
    for i in range(4):
        s.step(i)
    want = s.latents()
    s.close()
    assert _same(out, want)
    assert not _same(out, tsd_mod.generate(d, None, ctx, **kw))
    with pytest.raises(ValueError):
        tsd_mod.generate(d, None, ctx, controlnet=cn, **kw)


# ---- 6. the jitter build ----------------------------------------------------------------------------------------------------------------
def jitter_cases(tsd_mod, repeats):
    """[(name, [digest per repeat])]: the injection table of test 1 and one controlled forward at L = 16 (reference kind)."""
    xs, rs, groups, nslab = inject_table()
    table = []
    for _ in range(repeats):
        ys, ps = tsd_mod.control_inject(xs, rs, TABLE_SCALES, groups, nslab)
        table.append(_digest(ys + ps))
    cn_kind, unet_kind, _ = VARIANTS["reference"]
    cn = tsd_mod.ControlNet(params=R.draw_params(tsd_mod.param_specs(cn_kind), CN_SEED, nonzero=NONZERO), variant=cn_kind)
    d = tsd_mod.Diffusion(seed=SEED, variant=unet_kind)
    lat, ctx, temb, hint = _inputs(2, 16, 16, 700)
    fwd = [_digest([d.forward(lat, ctx, temb, control=cn, hint=hint, control_scale=SCALES)]) for _ in range(repeats)]
    cn.model.close(); d.model.close()
    return [("inject_table", table), ("controlled_forward_l16", fwd)]


def test_jitter_build_reproduces_the_shipped_bits(tsd_mod, gpu_ctx):
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    here = jitter_cases(tsd_mod, 1)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [r["name"] for r in there] == [n for n, _ in here]
    for (name, mine), theirs in zip(here, there):
        assert len(theirs["digests"]) == JITTER_REPEATS
        assert all(dg == mine[0] for dg in theirs["digests"]), f"{name}: the jitter build gave {len(set(theirs['digests']))} result(s), not the shipped bits"


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    import tsd
    tsd.set_strict(True)
    for _name, _digests in jitter_cases(tsd, int(sys.argv[2])):
        print(json.dumps({"name": _name, "digests": _digests}), flush=True)
