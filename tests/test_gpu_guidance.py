"""GPU tests of guidance rescale (include/tsd.h "guidance rescale"): the two launches against the fp64 reference (tests/guidance_ref.py), their
invariance (batch size, position, run, the -DTSD_JITTER build), degenerate inputs, the lockstep session against the host-driven loop, the
launch accounting when it is off, and slot sessions against lockstep sessions.
Session tests: Tiny-SD at random init (seed 1234), L = 8, T = 77, 1000 training steps, 4 inference steps, B = 3, CFG."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import guidance_ref as gr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
N_TRAIN, STEPS = 1000, 4
B, L, T = 3, 8, 77
CHW = 4 * L * L
SAMPLERS = [("ddpm", 0.0, "leading"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")]
IDS = ["ddpm", "ddim", "dpmpp_2m"]
SIZES = [4, 252, 256, 260, 2304, 16384]   # fewer elements than lanes; tails either side of a block; two partials per sample; the workload's
PHIS = (0.7, 0.0, 0.3, 1.0)               # row b of a call takes PHIS[b % 4]: mixed within one call, row 0 is on
FAMILIES = ["independent", "near", "offset"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


# ---- inputs and the reference, made once per (family, size) for 16 samples; a call of B samples takes the first B ---------------------------
_CASES = {}


def _case(tsd_mod, family, chw):
    key = (family, chw)
    if key not in _CASES:
        tag = 2100 + 10 * SIZES.index(chw)
        z = [tsd_mod.rng.normal(SEED, tag + k, 16 * chw).reshape(16, chw).astype(np.float32) for k in range(2)]
        if family == "independent":
            c, u = z
        elif family == "near":
            c, u = z[0], (z[0] + np.float32(0.1) * z[1]).astype(np.float32)
        else:
            c, u = ((np.float32(0.1) + np.float32(0.01) * v).astype(np.float32) for v in z)
        s = np.full(16, 7.5, dtype=np.float32)
        phi = np.array([PHIS[b % 4] for b in range(16)], dtype=np.float32)
        co, uo, g32, g64, kappa = gr.rescale(c, u, s, phi)
        for a in (c, u, co, uo, g32, kappa):
            a.setflags(write=False)
        _CASES[key] = dict(c=c, u=u, s=s, phi=phi, co=co, uo=uo, g32=g32, kappa=kappa)
    return _CASES[key]


# ---- 1. the kernels against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3, 16])
@pytest.mark.parametrize("family,chw", [(f, n) for f in FAMILIES[:2] for n in SIZES] + [("offset", 16384)])
def test_kernels_against_the_fp64_reference(gpu_ctx, tsd_mod, family, chw, nb):
    """The inputs' condition, from the reference alone: n 2^-53 kappa < 2^-30, so no float64 summation order can move g by a visible amount
    (the offset family, kappa about 102, is what an fp32 accumulation misses by a thousand ulps).  Then g within ONE float32 ulp of the
    reference's g rounded to float32 - the one ulp is for a final rounding that lands beside a tie, not a measured margin - the outputs
    bitwise float32(g_out) * c and float32(g_out) * u, and the rows at phi = 0 bitwise the inputs."""
    k = _case(tsd_mod, family, chw)
    on = k["phi"][:nb] > 0
    assert on[0] and (chw * 2.0 ** -53 * k["kappa"][:nb][on] < 2.0 ** -30).all(), k["kappa"][:nb]
    c, u = k["c"][:nb], k["u"][:nb]
    co, uo, g = tsd_mod.cfg_rescale(c, u, k["s"][:nb], k["phi"][:nb], ctx=gpu_ctx)
    ulps = gr.ulps_f32(g, k["g32"][:nb])
    print(f"[guidance] {family} chw={chw} B={nb}: g {g[:4].tolist()}  ulps from the reference {ulps.max()}  kappa {k['kappa'][:nb][on].max():.1f}")
    assert (g > 0).all() and np.isfinite(g).all()
    assert (ulps <= 1).all(), (ulps.tolist(), g.tolist(), k["g32"][:nb].tolist())
    assert np.array_equal(_bits(co), _bits(g[:, None] * c)) and np.array_equal(_bits(uo), _bits(g[:, None] * u))
    assert (g[~on] == 1.0).all() and np.array_equal(_bits(co[~on]), _bits(c[~on])) and np.array_equal(_bits(uo[~on]), _bits(u[~on]))
    assert (g[on] != 1.0).all()


# ---- 2. invariance ----------------------------------------------------------------------------------------------------------------------
def _digest(tsd_mod, ctx=None):
    """sha1 over g and both outputs of one call per size (3 samples each, mixed phi): what a library computes, for comparing two of them."""
    h = hashlib.sha1()
    for family, chw in (("independent", 4), ("near", 260), ("independent", 2304), ("offset", 16384)):
        k = _case(tsd_mod, family, chw)
        for a in tsd_mod.cfg_rescale(k["c"][:3], k["u"][:3], k["s"][:3], k["phi"][:3], ctx=ctx):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("chw", SIZES)
def test_a_sample_is_the_same_alone_and_in_a_batch_and_run_to_run(gpu_ctx, tsd_mod, chw):
    """Sample 2 of the case (phi = 0.3) alone at B = 1 and at position 2 of B = 3, and the B = 3 call twice: g and both outputs bitwise."""
    k = _case(tsd_mod, "independent", chw)
    three = [tsd_mod.cfg_rescale(k["c"][:3], k["u"][:3], k["s"][:3], k["phi"][:3], ctx=gpu_ctx) for _ in range(2)]
    alone = tsd_mod.cfg_rescale(k["c"][2:3], k["u"][2:3], k["s"][2:3], k["phi"][2:3], ctx=gpu_ctx)
    for a, b, one in zip(three[0], three[1], alone):
        assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(a[2]), _bits(one[0]))
    assert three[0][2][2] != 1.0


def test_the_jitter_build_computes_the_shipped_bits(gpu_ctx, tsd_mod):
    """The -DTSD_JITTER library (a random delay before the barrier of k_cfg_moments), in a process of its own like
    test_jitter_build_reproduces_the_shipped_bits loads it: the same digest as the shipped library in this process."""
    jit = os.path.join(ROOT, "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
    if not os.path.exists(jit):
        pytest.skip(f"{jit} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    here = _digest(tsd_mod, gpu_ctx)
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import tsd, test_gpu_guidance as t; tsd.set_strict(True); print('digest', t._digest(tsd))"
            % (ROOT, os.path.join(ROOT, "stable-diffusion.mojo_amd"), os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TSD_LIB=jit), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.split("digest")[-1].strip() == here, out.stdout[-500:]


# ---- 3. degenerate inputs ---------------------------------------------------------------------------------------------------------------
def test_constant_and_nan_inputs_pass_through(gpu_ctx, tsd_mod):
    chw = 2304
    k = _case(tsd_mod, "independent", chw)
    const = np.full((2, chw), 0.37, dtype=np.float32)
    co, uo, g = tsd_mod.cfg_rescale(const, const, 7.5, 0.7, ctx=gpu_ctx)
    assert (g == 1.0).all() and np.array_equal(_bits(co), _bits(const)) and np.array_equal(_bits(uo), _bits(const))
    c, u = k["c"][:3].copy(), k["u"][:3].copy()
    c[1, 777] = np.nan
    phi = np.array([0.7, 0.7, 0.3], dtype=np.float32)
    co, uo, g = tsd_mod.cfg_rescale(c, u, 7.5, phi, ctx=gpu_ctx)
    ro, _, rg, _, _ = gr.rescale(c, u, 7.5, phi)
    assert g[1] == 1.0 and np.isnan(co[1, 777]) and np.array_equal(_bits(np.delete(co[1], 777)), _bits(np.delete(c[1], 777)))
    assert np.array_equal(_bits(uo[1]), _bits(u[1]))
    for b in (0, 2):   # the others are what they are without the NaN next to them
        assert g[b] != 1.0 and gr.ulps_f32(g[b], rg[b]) <= 1 and np.array_equal(_bits(co[b]), _bits(g[b] * c[b])), b
    clean = tsd_mod.cfg_rescale(k["c"][:3], k["u"][:3], 7.5, phi, ctx=gpu_ctx)
    assert np.array_equal(_bits(clean[2][[0, 2]]), _bits(g[[0, 2]])) and np.array_equal(_bits(clean[0][[0, 2]]), _bits(co[[0, 2]]))


# ---- session helpers ----------------------------------------------------------------------------------------------------------------------
class hoist:
    """The context's switch for the sessions created inside; restored on exit (the context is shared by the whole run)."""

    def __init__(self, tsd_mod, gpu_ctx, on):
        self.lib, self.h, self.on = tsd_mod._lib.lib(), gpu_ctx.h, int(on)

    def __enter__(self):
        self.prev = self.lib.tsd_debug_set_session_hoist(self.h, self.on)
        assert self.prev in (0, 1)

    def __exit__(self, *exc):
        self.lib.tsd_debug_set_session_hoist(self.h, self.prev)


_FILL = {}


def _filler(tsd_mod):
    if not _FILL:
        _FILL["lat"] = tsd_mod.rng.normal(SEED, 2290, B * CHW).reshape(B, 4, L, L).astype(np.float32)
        _FILL["ctx"] = tsd_mod.rng.normal(SEED, 2291, B * T * 768).reshape(B, T, 768).astype(np.float32)
        _FILL["uctx"] = tsd_mod.rng.normal(SEED, 2292, B * T * 768).reshape(B, T, 768).astype(np.float32)
    return _FILL


def _request(tsd_mod, k):
    n = T * 768
    return dict(ctx=tsd_mod.rng.normal(SEED, 2300 + 10 * k, n).reshape(T, 768).astype(np.float32),
                uctx=tsd_mod.rng.normal(SEED, 2301 + 10 * k, n).reshape(T, 768).astype(np.float32), seed=1000003 * (k + 1) + 29,
                scale=(7.5, 9.0, 5.0)[k % 3], lat=tsd_mod.rng.normal(SEED, 2302 + 10 * k, CHW).reshape(4, L, L).astype(np.float32))


def _session(tsd_mod, model, sampler, nb=B, cfg=True):
    s = tsd_mod.Session(model, None, nb, L, T, cfg=cfg)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, STEPS, 0)
    return s


def _coeffs(tsd_mod, kind, eta, spacing, i, have_history):
    out = (C.c_double * 8)()
    r = tsd_mod._lib.lib().tsd_sampler_coeffs(tsd_mod._lib.sampler_kind(kind), float(eta), tsd_mod._lib.timestep_spacing(spacing), N_TRAIN, STEPS, 0,
                                              i, int(have_history), out)
    assert r == 0
    return np.array(out[:], dtype=np.float64)


def _sampler_step(tsd_mod, gpu_ctx, x, e_c, e_u, scale, hist, noise, c, keep_hist):
    from tsd._lib import check, f32, ptr
    x, e_c, e_u = f32(x), f32(e_c), f32(e_u)
    out, h = np.empty_like(x), (np.empty_like(x) if keep_hist else None)
    check(tsd_mod._lib.lib().tsd_sampler_step_f32(gpu_ctx.h, ptr(x), ptr(e_c), ptr(e_u), float(scale), ptr(f32(hist)) if hist is not None else None,
                                                  ptr(f32(noise)) if noise is not None else None, x.size, ptr(np.ascontiguousarray(c, dtype=np.float32)),
                                                  ptr(out), ptr(h)))
    return out, h


# ---- 4. the session against the host-driven loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [1, 0], ids=["hoist", "nohoist"])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=IDS)
def test_session_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, diffusion, sampler, on):
    """Per step, from the host: the UNet forward for cond and uncond, tsd.cfg_rescale on the two predictions, then the update op (the DDPM op
    or tsd_sampler_step_f32, the host keeping the DPM-Solver++(2M) history) with the noise a seeded session draws, tsd.normal_fill of stream
    16 + i.  The same kernels on the same scalars as step() with set_guidance_rescale(0.7): the latents after every step ARE the host loop's.
    (The session sums a sample's moments over the output convolution's layout and the op over CHW: another order of a float64 sum, which
    under the condition of test 1 does not reach the float32 g.)"""
    kind, eta, spacing = sampler
    f = _filler(tsd_mod)
    seeds = [41, 42, 43]
    scale, phi = 7.5, 0.7
    with hoist(tsd_mod, gpu_ctx, on):
        s = _session(tsd_mod, diffusion.model, sampler)
        s.upload(f["lat"], f["ctx"], f["uctx"], None, cfg_scale=scale)
        s.set_seeds(seeds)
        s.set_guidance_rescale(phi)
        assert s.guidance_rescale == np.float32(phi) and s.hoist_info()["active"] == on
        x, hist = f["lat"], None
        multistep = kind == "dpmpp_2m"
        gs = []
        for i in range(STEPS):
            s.step(i)
            got = s.latents()
            temb = np.repeat(tsd_mod.get_time_embedding(float(s.timestep(i))).reshape(1, 320), B, axis=0)
            e_c, e_u = diffusion.forward(x, f["ctx"], temb), diffusion.forward(x, f["uctx"], temb)
            e_c, e_u, g = tsd_mod.cfg_rescale(e_c, e_u, scale, phi, ctx=gpu_ctx)
            gs.append(g)
            noise = np.stack([tsd_mod.normal_fill(sd, 16 + i, CHW, ctx=gpu_ctx) for sd in seeds]).reshape(B, 4, L, L)
            if kind == "ddpm":
                x = tsd_mod.ddpm_step(x, e_c, e_u, scale, noise, i, STEPS, N_TRAIN, 0, spacing, ctx=gpu_ctx)
            else:
                cd = _coeffs(tsd_mod, kind, eta, spacing, i, hist is not None)
                assert int(cd[0]) == s.timestep(i)
                c = cd[2:].astype(np.float32)
                x, h = _sampler_step(tsd_mod, gpu_ctx, x, e_c, e_u, scale, hist, noise if c[5] != 0 else None, c, multistep)
                hist = h if multistep else None
            assert np.array_equal(_bits(got), _bits(x)), (sampler, on, i, float(np.abs(got - x).max()))
        s.close()
    gs = np.stack(gs)
    assert np.isfinite(gs).all() and (gs > 0).all() and (gs != 1.0).all(), gs


# ---- 5. no cost when off ------------------------------------------------------------------------------------------------------------------
def _counted(gpu_ctx, run_one, first, P=2):
    run_one(first)
    gpu_ctx.profile_begin()
    try:
        for i in range(first + 1, first + 1 + P):
            run_one(i)
    finally:
        prof = gpu_ctx.profile_end()
    return {k: n for k, (_, n) in prof.items()}


def test_a_session_that_is_off_runs_the_launches_and_bits_of_before(gpu_ctx, tsd_mod, diffusion):
    """Per-class launch counts over 2 steps and the latents, for a session never told, one told 0, one told 0.7 and then 0: identical.
    With 0.7 the 2 steps make at most 2 more elementwise launches each and nothing else - and other latents."""
    f = _filler(tsd_mod)
    sampler = SAMPLERS[0]

    def run(tell):
        s = _session(tsd_mod, diffusion.model, sampler)
        s.upload(f["lat"], f["ctx"], f["uctx"], None, cfg_scale=7.5)
        s.set_seeds([1, 2, 3])
        for phi in tell:
            s.set_guidance_rescale(phi)
        n = _counted(gpu_ctx, s.step, 0)
        lat = s.latents()
        s.close()
        return n, lat

    never, zero, back, on = run(()), run((0.0,)), run((0.7, 0.0)), run((0.7,))
    assert never[0] == zero[0] == back[0], (never[0], zero[0], back[0])
    assert np.array_equal(_bits(never[1]), _bits(zero[1])) and np.array_equal(_bits(never[1]), _bits(back[1]))
    extra = {k: on[0][k] - never[0][k] for k in never[0]}
    print(f"[guidance] launches per 2 steps: off {never[0]}, extra with phi = 0.7 {extra}")
    assert 0 < extra.pop("elementwise") <= 2 * 2 and not any(extra.values()), extra
    assert not np.array_equal(on[1], never[1]) and np.isfinite(on[1]).all()


def test_an_advance_with_no_rescaled_slot_runs_the_launches_and_bits_of_before(gpu_ctx, tsd_mod, diffusion):
    """The same comparison for advance(): slots never told, told 0, told 0.7 and then 0 - and with slot 1 at 0.7, at most 2 more elementwise
    launches per advance, nothing else, and the OTHER slots' latents bitwise what they were."""
    sampler = SAMPLERS[0]
    reqs = [_request(tsd_mod, k) for k in range(B)]

    def run(tell):
        s = _session(tsd_mod, diffusion.model, sampler)
        s.slots_open()
        for k in range(B):
            s.slot_start(k, reqs[k]["ctx"], reqs[k]["uctx"], seed=reqs[k]["seed"], cfg_scale=reqs[k]["scale"])
        for b, phi in tell:
            s.slot_set_guidance_rescale(b, phi)
        n = _counted(gpu_ctx, lambda i: s.advance(), 0)
        lat = s.raw_latents()
        s.close()
        return n, lat

    never, zero, back, on = run(()), run(((1, 0.0),)), run(((1, 0.7), (1, 0.0))), run(((1, 0.7),))
    assert never[0] == zero[0] == back[0], (never[0], zero[0], back[0])
    assert np.array_equal(_bits(never[1]), _bits(zero[1])) and np.array_equal(_bits(never[1]), _bits(back[1]))
    extra = {k: on[0][k] - never[0][k] for k in never[0]}
    assert 0 < extra.pop("elementwise") <= 2 * 2 and not any(extra.values()), extra
    assert np.array_equal(_bits(on[1][[0, 2]]), _bits(never[1][[0, 2]])) and not np.array_equal(on[1][1], never[1][1])


# ---- 6. slots -----------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _lockstep(tsd_mod, model, sampler, req, k, pos, phi, start=None):
    """Sample `pos` of a lockstep B = 3 session running request k there with its cfg_scale and guidance rescale phi (made once per case)."""
    key = (sampler, k, pos, float(phi), start)
    if key not in _REF:
        f = _filler(tsd_mod)
        lat, ctx, uctx = f["lat"].copy(), f["ctx"].copy(), f["uctx"].copy()
        ctx[pos], uctx[pos] = req["ctx"], req["uctx"]
        if start is not None:
            lat[pos] = req["lat"]
        seeds = [91, 92, 93]
        seeds[pos] = req["seed"]
        s = _session(tsd_mod, model, sampler)
        s.upload(lat, ctx, uctx, None, cfg_scale=req["scale"])
        s.set_seeds(seeds)
        if start is None:
            s.seed_latents()
        else:
            s.add_noise_seeded(start)
        if phi > 0:
            s.set_guidance_rescale(phi)
        for i in range(start or 0, STEPS):
            s.step(i)
        _REF[key] = s.latents()[pos].copy()
        s.close()
    return _REF[key]


SLOT_PHIS = (0.0, 0.7, 0.3)


@pytest.mark.parametrize("sampler", SAMPLERS, ids=IDS)
def test_staggered_slots_equal_lockstep_bitwise(gpu_ctx, tsd_mod, diffusion, sampler):
    """Request k starts in slot k after k advances with guidance rescale (0, 0.7, 0.3)[k]: slot_latents(k) == sample k of the lockstep session
    of request k with that phi, bit for bit - and the rescaled ones differ from their own phi = 0 run.  When slot 0 is done it is refilled:
    the new request has phi = 0 and finishes on its phi = 0 reference."""
    reqs = [_request(tsd_mod, k) for k in range(4)]
    s = _session(tsd_mod, diffusion.model, sampler)
    s.slots_open()
    got = {}
    for tick in range(6):
        if tick < B:
            r = reqs[tick]
            s.slot_start(tick, r["ctx"], r["uctx"], seed=r["seed"], cfg_scale=r["scale"])
            assert s.slot_guidance_rescale(tick) == 0.0
            if SLOT_PHIS[tick] > 0:
                s.slot_set_guidance_rescale(tick, SLOT_PHIS[tick])
            assert s.slot_guidance_rescale(tick) == np.float32(SLOT_PHIS[tick])
        for b in s.advance():
            got[(b, tick)] = s.slot_latents(b)
        if tick == 3:   # slot 0 is done while 1 and 2 run at 0.7 and 0.3: refill it (img2img from index 2)
            assert (0, 3) in got and s.slot_guidance_rescale(1) == np.float32(0.7)
            r = reqs[3]
            s.slot_start(0, r["ctx"], r["uctx"], latents=r["lat"], noise_at_start=True, seed=r["seed"], start_index=2, cfg_scale=r["scale"])
            assert s.slot_guidance_rescale(0) == 0.0 and s.slot_state(0) == (2, s.SLOT_ACTIVE)
            s.slot_set_guidance_rescale(0, 0.3)
            s.slot_start(0, r["ctx"], r["uctx"], latents=r["lat"], noise_at_start=True, seed=r["seed"], start_index=2, cfg_scale=r["scale"])
            assert s.slot_guidance_rescale(0) == 0.0   # a refilled slot never inherits it
    assert sorted(got) == [(0, 3), (0, 5), (1, 4), (2, 5)] and s.slots_active() == 0
    s.close()
    for k in range(B):
        ref = _lockstep(tsd_mod, diffusion.model, sampler, reqs[k], k, k, SLOT_PHIS[k])
        mine = got[(k, 3 + k)]
        assert np.isfinite(mine).all() and np.array_equal(_bits(mine), _bits(ref)), (k, float(np.abs(mine - ref).max()))
        if SLOT_PHIS[k] > 0:
            assert not np.array_equal(ref, _lockstep(tsd_mod, diffusion.model, sampler, reqs[k], k, k, 0.0))
    refill = _lockstep(tsd_mod, diffusion.model, sampler, reqs[3], 3, 0, 0.0, start=2)
    assert np.array_equal(_bits(got[(0, 5)]), _bits(refill)), float(np.abs(got[(0, 5)] - refill).max())


def test_idle_and_done_slots_are_not_written(gpu_ctx, tsd_mod, diffusion):
    """Slot 0 starts at index 2 and is done after two advances, slot 1 runs on at phi = 0.7, slot 2 stays idle: over two further advances the
    done slot's and the idle slot's latents keep their bits while the active slot's change."""
    reqs = [_request(tsd_mod, k) for k in range(2)]
    s = _session(tsd_mod, diffusion.model, SAMPLERS[0])
    s.slots_open()
    s.slot_start(0, reqs[0]["ctx"], reqs[0]["uctx"], latents=reqs[0]["lat"], noise_at_start=True, seed=reqs[0]["seed"], start_index=2)
    s.slot_start(1, reqs[1]["ctx"], reqs[1]["uctx"], seed=reqs[1]["seed"])
    s.slot_set_guidance_rescale(0, 0.7)
    s.slot_set_guidance_rescale(1, 0.7)
    assert s.advance() == [] and s.advance() == [0]
    assert s.slot_guidance_rescale(0) == 0.0   # done: nothing in force
    before = s.raw_latents()
    assert s.slot_state(2) == (0, s.SLOT_IDLE) and not before[2].any()
    assert s.advance() == [] and s.advance() == [1]
    after = s.raw_latents()
    assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(_bits(after[2]), _bits(before[2]))
    assert not np.array_equal(after[1], before[1]) and np.isfinite(after).all()
    s.close()


def test_state_machine(gpu_ctx, tsd_mod, diffusion):
    from tsd._lib import TSD_E_ARG, TSD_E_STATE, TSD_OK
    lib = tsd_mod._lib.lib()
    f = _filler(tsd_mod)
    r = _request(tsd_mod, 0)
    phi = C.c_float(-1.0)

    def value(s):
        assert lib.tsd_session_guidance_rescale(s.h, C.byref(phi)) == TSD_OK
        return phi.value

    s = _session(tsd_mod, diffusion.model, SAMPLERS[1])
    assert lib.tsd_session_set_guidance_rescale(s.h, 0.7) == TSD_E_STATE and value(s) == 0.0          # before upload()
    assert lib.tsd_session_slot_set_guidance_rescale(s.h, 0, 0.7) == TSD_E_STATE                       # not in slot mode
    assert lib.tsd_session_slot_guidance_rescale(s.h, 0, C.byref(phi)) == TSD_E_STATE
    s.upload(f["lat"], f["ctx"], f["uctx"], None)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert lib.tsd_session_set_guidance_rescale(s.h, bad) == TSD_E_ARG, bad
    assert value(s) == 0.0
    assert lib.tsd_session_set_guidance_rescale(s.h, 0.7) == TSD_OK and value(s) == np.float32(0.7)
    assert lib.tsd_session_set_guidance_rescale(s.h, 2.0) == TSD_E_ARG and value(s) == np.float32(0.7)   # a refusal leaves it
    # it touches neither the latents nor the history: a DPM-Solver++(2M) session told between two steps equals the host's idea of it in
    # test 4; here: upload(), set_schedule and set_sampler turn it off
    s.upload(f["lat"], f["ctx"], f["uctx"], None)
    assert value(s) == 0.0
    s.set_guidance_rescale(1.0)
    s.set_schedule(N_TRAIN, STEPS, 0)
    assert value(s) == 0.0 and lib.tsd_session_set_guidance_rescale(s.h, 0.7) == TSD_E_STATE
    s.upload(f["lat"], f["ctx"], f["uctx"], None)
    s.set_guidance_rescale(0.5)
    s.set_sampler(*SAMPLERS[2])
    assert value(s) == 0.0
    # slot mode: the lockstep setter is closed; the slot setter belongs to an active slot
    s.slots_open()
    assert lib.tsd_session_set_guidance_rescale(s.h, 0.7) == TSD_E_STATE
    assert lib.tsd_session_slot_set_guidance_rescale(s.h, 0, 0.7) == TSD_E_STATE                       # idle
    assert lib.tsd_session_slot_set_guidance_rescale(s.h, B, 0.7) == TSD_E_ARG and lib.tsd_session_slot_set_guidance_rescale(s.h, -1, 0.7) == TSD_E_ARG
    assert lib.tsd_session_slot_guidance_rescale(s.h, B, C.byref(phi)) == TSD_E_ARG
    s.slot_start(0, r["ctx"], r["uctx"], seed=r["seed"])
    for bad in (-0.1, 1.5, float("nan")):
        assert lib.tsd_session_slot_set_guidance_rescale(s.h, 0, bad) == TSD_E_ARG, bad
    assert s.slot_guidance_rescale(0) == 0.0
    s.slot_set_guidance_rescale(0, 0.7)
    assert s.slot_guidance_rescale(0) == np.float32(0.7) and s.slot_guidance_rescale(1) == 0.0
    s.slots_open()   # clears every slot
    assert s.slot_guidance_rescale(0) == 0.0
    s.close()
    # a session without CFG has nothing to rescale
    n = _session(tsd_mod, diffusion.model, SAMPLERS[0], cfg=False)
    n.upload(f["lat"], f["ctx"], None, None)
    assert lib.tsd_session_set_guidance_rescale(n.h, 0.7) == TSD_E_STATE and lib.tsd_session_set_guidance_rescale(n.h, 0.0) == TSD_E_STATE
    n.slots_open()
    n.slot_start(0, r["ctx"], None, seed=r["seed"])
    assert lib.tsd_session_slot_set_guidance_rescale(n.h, 0, 0.7) == TSD_E_STATE
    n.close()


def test_generate_stream_gives_a_rescaled_request_what_generate_gives_it(gpu_ctx, tsd_mod, diffusion):
    """Three requests through B = 2, the second with guidance_rescale = 0.7: each equals generate(..., guidance_rescale=..., seeds=...) at
    B = 2 for the request in the sample position the scheduler put it in."""
    from tsd.serve import Request, generate_stream
    nb, steps = 2, 3
    reqs = [_request(tsd_mod, k) for k in range(3)]
    phis = (0.0, 0.7, 0.0)
    out = dict(generate_stream(diffusion, None, (Request(k, r["ctx"], r["uctx"], r["seed"], r["scale"], guidance_rescale=phis[k])
                                                 for k, r in enumerate(reqs)), nb, L, T, cfg=True, inference_steps=steps, num_training_steps=N_TRAIN))
    assert sorted(out) == [0, 1, 2]
    f = _filler(tsd_mod)
    for k, r in enumerate(reqs):
        pos = k % nb
        ctx, uctx = f["ctx"][:nb].copy(), f["uctx"][:nb].copy()
        ctx[pos], uctx[pos] = r["ctx"], r["uctx"]
        seeds = [5, 6]
        seeds[pos] = r["seed"]
        ref = [tsd_mod.generate(diffusion, None, ctx, uncond_context=uctx, cfg=True, cfg_scale=r["scale"], inference_steps=steps,
                                num_training_steps=N_TRAIN, L=L, seeds=seeds, guidance_rescale=p)[pos] for p in (phis[k], 0.7 - phis[k])]
        assert np.isfinite(out[k]).all() and np.array_equal(_bits(out[k]), _bits(ref[0])), (k, float(np.abs(out[k] - ref[0]).max()))
        assert not np.array_equal(ref[0], ref[1])   # the argument reaches the steps
