"""GPU: the SD-2.x model kinds - "diffusion_sd2" (kind 16: the full-size graph with head dimension 64 in every attention block and a
1024-wide context) and "clip_sd2" (kind 17: the OpenCLIP-H text encoder, width 1024, 16 heads, 23 layers, erf-GELU).

* the UNet forward against numpy (tests/sd2_ref.py: the oracle's block functions over the SD-2 step table) at B = 2, latents 16x16, 16x32
  and 32x16 (the smallest sides the graph allows: 256 / 64 / 16 / 4 tokens - or their rectangular counterparts - and 77 context keys),
  timesteps 980 and 20, within the project's bound for a whole model (TOL_MODEL, TOL_MODEL_MAX of tests/util.py);
* the text encoder on two prompts, one of them 77 tokens long, against the restatement at TOL_MODEL;
* bitwise: run to run, a sample alone against its row of B = 3, key-map round trips (proj_in stored 2-D and 4-D; the text encoder), a
  session against a host-driven loop at 16x16 with B = 2 (seeded DDPM; DPM-Solver++(2M); v-prediction with the zero-terminal-SNR table on a
  trailing list; CFG on and off; hoist on and off; inpainting and guidance rescale together), a slot session against the lockstep session of
  the same requests, and the jitter build's UNet forward;
* refusals: a ControlNet on an SD-2 UNet (forward and session), a 768-wide context handed to an SD-2 session or forward.

Parameters are drawn from tsd.param_specs(kind) with a seed (sd2_ref.draw_params) and handed to both sides.

Measured on an MI355X, relative L2 / max error over max |ref|: UNet forward 16x16 1.28e-3 / 1.36e-3 (t = 980) and
1.25e-3 / 1.07e-3 (t = 20), 16x32 1.21e-3 / 1.30e-3 and 1.26e-3 / 1.26e-3, 32x16 1.22e-3 / 1.45e-3 and 1.29e-3 / 1.41e-3 (bound 1e-2 /
1.2e-2); text encoder 1.37e-3 / 2.23e-3 (9 tokens) and 1.44e-3 / 2.72e-3 (77 tokens) (bound 1e-2 relative L2).

Run as `python tests/test_gpu_sd2.py jitter-child REPEATS` this file is the child of the jitter test: it prints one JSON line of digests on
whatever library TSD_LIB names."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (_ROOT, os.path.join(_ROOT, "stable-diffusion.mojo_amd"), os.path.dirname(os.path.abspath(__file__))):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import pytest

import inpaint_ref as IR
import sd2_ref as R
from oracle import ops, rng
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, max_rel, rel_l2

pytestmark = pytest.mark.gpu
SEED, T, W = 1234, 77, 1024
N_TRAIN = 1000
KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}
SPACINGS = {"leading": 0, "trailing": 1}
JITTER_LIB = os.path.join(_ROOT, "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
JITTER_REPEATS = 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def unet_p(tsd_mod):
    return R.draw_params(tsd_mod.param_specs("diffusion_sd2"), 11)


@pytest.fixture(scope="module")
def unet(gpu_ctx, tsd_mod, unet_p):
    m = tsd_mod.Diffusion(params=unet_p, variant="diffusion_sd2")
    yield m
    m.model.close()


@pytest.fixture(scope="module")
def clip_p(tsd_mod):
    return R.draw_params(tsd_mod.param_specs("clip_sd2"), 12)


@pytest.fixture(scope="module")
def clip(gpu_ctx, tsd_mod, clip_p):
    m = tsd_mod.CLIP(params=clip_p, variant="clip_sd2")
    yield m
    m.model.close()


def _inputs(B, L, tag, width=W):
    LH, LW = (L, L) if isinstance(L, int) else L
    lat = rng.normal(SEED, tag, B * 4 * LH * LW).reshape(B, 4, LH, LW)
    ctx = rng.normal(SEED, tag + 1, B * T * width).reshape(B, T, width)
    uctx = rng.normal(SEED, tag + 2, B * T * width).reshape(B, T, width)
    return lat, ctx, uctx


# ---- 1. models against numpy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [980, 20])
@pytest.mark.parametrize("L", [(16, 16), (16, 32), (32, 16)], ids=["16x16", "16x32", "32x16"])
def test_unet_forward_matches_numpy(tsd_mod, unet, unet_p, L, t):
    B = 2
    lat, ctx, _ = _inputs(B, L, 2100 + t)
    assert unet.model.context_width == W
    temb = tsd_mod.get_time_embedding(float(t)).reshape(1, 320)
    out = unet.forward(lat, ctx, np.repeat(temb, B, axis=0))
    ref = np.stack([R.diffusion_sd2(unet_p, lat[b], ctx[b], ops.time_embedding(float(t))) for b in range(B)])
    print(f"[sd2] UNet forward {L[0]}x{L[1]} t={t}: rel_l2 {rel_l2(out, ref):.3e} max {max_rel(out, ref):.3e}")
    assert out.shape == lat.shape and np.isfinite(out).all()
    assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, f"SD-2 UNet {L} t={t}")


def test_text_encoder_matches_numpy(tsd_mod, clip, clip_p):
    g = np.random.default_rng(5)
    short, full = g.integers(1, 49408, 9), g.integers(1, 49408, 77)
    assert clip.model.context_width == W
    for name, ids in (("9 tokens", short), ("77 tokens", full)):
        out = clip.forward(ids)
        ref = R.clip_sd2(clip_p, ids)
        print(f"[sd2] text encoder {name}: rel_l2 {rel_l2(out, ref):.3e} max {max_rel(out, ref):.3e}")
        assert out.shape == (77, W) and np.isfinite(out).all()
        assert_close(out, ref, TOL_MODEL, None, f"SD-2 text encoder, {name}")
    both = np.zeros((2, 77), np.int32)                       # ids past the prompt are 0: the batch of both is each alone
    both[0, :9], both[1] = short, full
    ob = clip.forward(both)
    assert _same(ob[0], clip.forward(short)) and _same(ob[1], clip.forward(full))


# ---- 2. bitwise properties -------------------------------------------------------------------------------------------------------------
def test_unet_run_to_run_and_batch_invariance_are_bitwise(tsd_mod, unet):
    lat, ctx, _ = _inputs(3, 16, 2200)
    temb = np.repeat(tsd_mod.get_time_embedding(500.0).reshape(1, 320), 3, axis=0)
    y3 = unet.forward(lat, ctx, temb)
    assert _same(y3, unet.forward(lat, ctx, temb))
    for b in range(3):
        assert _same(unet.forward(lat[b], ctx[b], temb[b]), y3[b]), b


def test_unet_key_map_round_trip_loads_the_same_model(tsd_mod, gpu_ctx, unet, unet_p):
    """params -> diffusers names (proj_in / proj_out 2-D as the SD-2.x files hold them, and 4-D) -> params: the dict of the directly
    initialised model; the model loaded from the 2-D state dict computes the same bits."""
    from tsd import checkpoint as ck
    for linear in (True, False):
        state = ck.params_to_diffusers_sd2_unet(unet_p, linear_projection=linear)
        assert state["down_blocks.0.attentions.0.proj_in.weight"].ndim == (2 if linear else 4)
        back = ck.diffusers_sd2_unet_to_params(state)
        assert set(back) == set(unet_p)
        assert all(back[k].shape == unet_p[k].shape and np.array_equal(back[k], unet_p[k]) for k in unet_p), linear
    m2 = ck.load_sd2_unet(ck.params_to_diffusers_sd2_unet(unet_p, linear_projection=True), ctx=gpu_ctx)
    try:
        assert m2.model.kind == tsd_mod._lib.MODEL_DIFFUSION_SD2
        lat, ctx, _ = _inputs(1, 16, 2210)
        temb = tsd_mod.get_time_embedding(300.0).reshape(1, 320)
        assert _same(m2.forward(lat, ctx, temb), unet.forward(lat, ctx, temb))
    finally:
        m2.model.close()


def test_text_encoder_key_map_round_trip_loads_the_same_model(tsd_mod, gpu_ctx, clip, clip_p):
    from tsd import checkpoint as ck
    state = ck.params_to_hf_clip_text(clip_p)
    assert "text_model.encoder.layers.22.mlp.fc1.weight" in state and "text_model.encoder.layers.23.mlp.fc1.weight" not in state
    back = ck.hf_clip_text_to_params(state)
    assert set(back) == set(clip_p) and all(np.array_equal(back[k].reshape(clip_p[k].shape), clip_p[k]) for k in clip_p)
    m2 = ck.load_clip_text(state, ctx=gpu_ctx)
    try:
        assert m2.model.kind == tsd_mod._lib.MODEL_CLIP_SD2
        ids = np.arange(100, 140)
        assert _same(m2.forward(ids), clip.forward(ids))
    finally:
        m2.model.close()


# ---- 3. a session against a host-driven loop --------------------------------------------------------------------------------------------
def coeffs_ex(tsd_mod, kind, eta, spacing, n, i, have_history, pred, ztsnr):
    out = (C.c_double * 8)()
    rc = tsd_mod._lib.lib().tsd_sampler_coeffs_ex(KINDS[kind], float(eta), SPACINGS[spacing], N_TRAIN, n, 0, i, int(have_history),
                                                  tsd_mod._lib.PREDICTION_TYPES[pred], int(ztsnr), out)
    assert rc == 0, tsd_mod._lib.last_error()
    return np.array(out[:], dtype=np.float64)


class Hoist:
    """tsd_debug_set_session_hoist on the default context for the body of a `with`."""

    def __init__(self, tsd_mod, gpu_ctx, on):
        self.lib, self.h, self.on = tsd_mod._lib.lib(), gpu_ctx.h, int(on)

    def __enter__(self):
        self.prev = self.lib.tsd_debug_set_session_hoist(self.h, self.on)
        assert self.prev in (0, 1)

    def __exit__(self, *exc):
        self.lib.tsd_debug_set_session_hoist(self.h, self.prev)


def _mask(B, L):
    m = np.zeros((B, L, L), dtype=np.float32)
    m[:, :, : L // 2 - 1] = 1.0
    m[:, :, L // 2 - 1] = 0.75
    m[:, :, L // 2] = 0.3
    for b in range(B):
        m[b, b] = 1.0 - m[b, b]
    return m


def run_both(tsd_mod, gpu_ctx, unet, sampler, cfg, pred, ztsnr, tag, seeds=None, phi=0.0, inpaint=False, steps=3, B=2, L=16):
    """The session's latents after every step against the host loop's, bitwise: UNet forward from the host on the device-computed time
    embedding, [guidance rescale,] the update op with the session's scalars (tsd_ddpm_step_f32 for an epsilon DDPM session, else
    tsd_sampler_step_f32 / tsd_sampler_step_v_f32 with the host keeping the history), [the inpainting blend]."""
    kind, eta, spacing = sampler
    lat, ctx, uctx = _inputs(B, L, tag)
    known, z = (rng.normal(SEED, tag + k, lat.size).reshape(lat.shape) for k in (5, 6))
    chw = lat[0].size
    nz = rng.normal(SEED, tag + 3, steps * lat.size).reshape((steps,) + lat.shape)
    s = tsd_mod.Session(unet.model, None, B, L, T, cfg=cfg)
    assert s.W == W
    s.set_prediction(pred, ztsnr)
    s.set_sampler(kind, eta, spacing)
    s.set_schedule(N_TRAIN, steps, 0)
    s.upload(lat, ctx, uctx if cfg else None, None if seeds else nz, cfg_scale=7.5)
    if seeds:
        s.set_seeds(seeds)
        nz = np.stack([np.stack([tsd_mod.normal_fill(sd, 16 + i, chw, ctx=gpu_ctx).reshape(lat[0].shape) for sd in seeds]) for i in range(steps)])
    if phi > 0.0:
        s.set_guidance_rescale(phi)
    if inpaint:
        s.set_inpaint(_mask(B, L), known, z)
    x, hist = lat, None
    multistep = kind == "dpmpp_2m"
    for i in range(steps):
        s.step(i)
        got = s.latents()
        cd = coeffs_ex(tsd_mod, kind, eta, spacing, steps, i, hist is not None, pred, ztsnr)
        t = int(cd[0])
        assert t == s.timestep(i)
        temb = np.repeat(tsd_mod.get_time_embedding(float(t)).reshape(1, 320), B, axis=0)
        o_c = unet.forward(x, ctx, temb)
        o_u = unet.forward(x, uctx, temb) if cfg else None
        if phi > 0.0:
            o_c, o_u, _ = tsd_mod.cfg_rescale(o_c, o_u, 7.5, phi, ctx=gpu_ctx)
        c6 = cd[2:].astype(np.float32)
        noise = nz[i] if c6[5] != 0 else None
        if pred == "v":
            x, h = tsd_mod.sampler_step_v(x, o_c, o_u, 7.5, hist, noise, c6, multistep, ctx=gpu_ctx)
        elif kind == "ddpm":
            x, h = tsd_mod.ddpm_step(x, o_c, o_u, 7.5, nz[i], i, steps, N_TRAIN, 0, spacing, ctx=gpu_ctx), None
        else:
            x, h = IR.step_f32(tsd_mod, gpu_ctx, x, o_c, o_u, 7.5, hist, noise, c6, multistep)
        hist = h if multistep else None
        if inpaint:
            if i + 1 < steps:
                nx = coeffs_ex(tsd_mod, kind, eta, spacing, steps, i + 1, 0, pred, ztsnr)
                a_prev, s_prev = np.float32(nx[2]), np.float32(nx[3])
            else:
                a_prev, s_prev = np.float32(1.0), np.float32(0.0)
            x = IR.blend_op(tsd_mod, gpu_ctx, x, _mask(B, L), known, z, a_prev, s_prev)
        assert np.isfinite(got).all()
        assert _same(got, x), (sampler, cfg, pred, i, float(np.abs(got - x).max()))
    s.close()


SESSION_CASES = {
    "seeded_ddpm_cfg": dict(sampler=("ddpm", 0.0, "leading"), cfg=True, pred="epsilon", ztsnr=False, seeds=[1234567, 89]),
    "dpmpp_2m_nocfg": dict(sampler=("dpmpp_2m", 0.0, "leading"), cfg=False, pred="epsilon", ztsnr=False),
    "v_ztsnr_trailing_cfg": dict(sampler=("ddpm", 0.0, "trailing"), cfg=True, pred="v", ztsnr=True),
    "v_ztsnr_trailing_nocfg": dict(sampler=("ddim", 0.5, "trailing"), cfg=False, pred="v", ztsnr=True),
    "inpaint_and_rescale": dict(sampler=("dpmpp_2m", 0.0, "trailing"), cfg=True, pred="v", ztsnr=True, phi=0.7, inpaint=True),
}


# every configuration with the hoist on (the default); one CFG and one non-CFG configuration with it off as well
SESSION_RUNS = [(n, 1) for n in sorted(SESSION_CASES)] + [("seeded_ddpm_cfg", 0), ("v_ztsnr_trailing_nocfg", 0)]


@pytest.mark.parametrize("name,hoist", SESSION_RUNS, ids=[f"{n}-{'hoist' if h else 'nohoist'}" for n, h in SESSION_RUNS])
def test_session_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, unet, name, hoist):
    with Hoist(tsd_mod, gpu_ctx, hoist):
        run_both(tsd_mod, gpu_ctx, unet, tag=2300 + 10 * sorted(SESSION_CASES).index(name), **SESSION_CASES[name])


def test_slot_session_equals_the_lockstep_session_of_the_same_requests(gpu_ctx, tsd_mod, unet):
    """Two requests started together in slots 0 and 1 against a lockstep session seeded with the same seeds: DPM-Solver++(2M), CFG,
    v-prediction on the zero-terminal-SNR table, 3 steps; bitwise."""
    B, L, steps = 2, 16, 3
    _, ctx, uctx = _inputs(B, L, 2400)
    seeds = [77, 1 << 40]

    def conf(s):
        s.set_prediction("v", True)
        s.set_sampler("dpmpp_2m", 0.0, "trailing")
        s.set_schedule(N_TRAIN, steps, 0)

    lock = tsd_mod.Session(unet.model, None, B, L, T, cfg=True)
    conf(lock)
    lock.upload(np.zeros((B, 4, L, L), np.float32), ctx, uctx, None, cfg_scale=6.0)
    lock.set_seeds(seeds)
    lock.seed_latents()
    for i in range(steps):
        lock.step(i)
    want = lock.latents()
    lock.close()
    s = tsd_mod.Session(unet.model, None, B, L, T, cfg=True)
    conf(s)
    s.slots_open()
    for b in range(B):
        s.slot_start(b, ctx[b], uctx[b], None, seed=seeds[b], cfg_scale=6.0)
    done = []
    for _ in range(steps):
        done += s.advance()
    assert sorted(done) == [0, 1]
    for b in range(B):
        assert _same(s.slot_latents(b), want[b]), b
    s.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_a_controlnet_on_an_sd2_unet_is_refused(gpu_ctx, tsd_mod, unet):
    cn = tsd_mod.ControlNet(seed=3, variant="controlnet_sd15_torch")
    try:
        lat, ctx, _ = _inputs(1, 16, 2500)
        temb = tsd_mod.get_time_embedding(100.0).reshape(1, 320)
        hint = np.zeros((3, 128, 128), np.float32)
        with pytest.raises(tsd_mod.TsdError) as e:
            unet.forward(lat, ctx, temb, control=cn, hint=hint)
        assert e.value.code == tsd_mod._lib.TSD_E_ARG and "1024" in str(e.value) and "768" in str(e.value)
        s = tsd_mod.Session(unet.model, None, 1, 16, T, cfg=False)
        s.set_schedule(N_TRAIN, 2, 0)
        s.upload(lat, ctx)
        with pytest.raises(tsd_mod.TsdError) as e:
            s.set_control(cn, hint)
        assert e.value.code == tsd_mod._lib.TSD_E_ARG and not s.control_active
        s.close()
    finally:
        cn.model.close()


def test_a_768_wide_context_is_refused_naming_both_widths(gpu_ctx, tsd_mod, unet):
    lat, ctx768, _ = _inputs(2, 16, 2510, width=768)
    s = tsd_mod.Session(unet.model, None, 2, 16, T, cfg=False)
    with pytest.raises(ValueError, match=r"1024.*768"):
        s.upload(lat, ctx768)
    s.slots_open()
    with pytest.raises(ValueError, match=r"1024.*768"):
        s.slot_start(0, ctx768[0])
    s.close()
    with pytest.raises(ValueError, match=r"1024"):
        unet.forward(lat, ctx768, np.zeros((2, 320), np.float32))


# ---- 5. the jitter build ---------------------------------------------------------------------------------------------------------------
def jitter_cases(tsd_mod, repeats):
    """[(name, [digest per repeat])]: one UNet forward of a seeded kind-16 model (B = 2, 16x16)."""
    m = tsd_mod.Diffusion(seed=5, variant="diffusion_sd2")
    lat, ctx, _ = _inputs(2, 16, 2600)
    temb = np.repeat(tsd_mod.get_time_embedding(640.0).reshape(1, 320), 2, axis=0)
    digs = [hashlib.sha256(_bits(m.forward(lat, ctx, temb)).tobytes()).hexdigest()[:16] for _ in range(repeats)]
    m.model.close()
    return [("unet_sd2_forward", digs)]


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
