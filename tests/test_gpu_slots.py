"""GPU tests of slot sessions: samples that join and leave a running denoise batch.  A slot's latents are held, bit for bit, to a lockstep
session of the same batch shape running the slot's request in the same sample position (so only the feature is under test): staggered
starts, a refill while others run, bystanders, launch accounting, the state machine and `generate_stream`.
Tiny-SD at random init (seed 1234), L = 8, T = 77, 1000 training steps, 4 inference steps."""
import ctypes as C

import numpy as np
import pytest

from oracle import rng

pytestmark = pytest.mark.gpu
SEED = 1234
N_TRAIN, STEPS = 1000, 4
B, L, T = 3, 8, 77
CHW = 4 * L * L
SAMPLERS = [("ddpm", 0.0, "leading"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing"), ("ddpm", 0.0, "trailing")]
IDS = ["ddpm", "ddim", "dpmpp_2m", "ddpm_trailing"]  # the last: DDPM's previous timestep from the list, the final step onto -1 with noise
SCALES = (7.5, 3.0, 1.0)
K_PROJ, T_PROJ = "unet.layer3.layer6.k_proj.weight", "unet.layer2.layer3.weight"


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _request(k):
    """Request k: its own context, uncond context, seed, guidance scale, and latents for when it is an img2img request."""
    return dict(ctx=rng.normal(SEED, 1500 + 10 * k, T * 768).reshape(T, 768), uctx=rng.normal(SEED, 1501 + 10 * k, T * 768).reshape(T, 768),
                seed=1000003 * (k + 1) + 17, scale=SCALES[k % 3], lat=rng.normal(SEED, 1502 + 10 * k, CHW).reshape(4, L, L))


_FILL = {}


def _filler():
    """Finite data for the other samples of a lockstep reference (made once)."""
    if not _FILL:
        _FILL["lat"] = rng.normal(SEED, 1490, B * CHW).reshape(B, 4, L, L)
        _FILL["ctx"] = rng.normal(SEED, 1491, B * T * 768).reshape(B, T, 768)
        _FILL["uctx"] = rng.normal(SEED, 1492, B * T * 768).reshape(B, T, 768)
    return _FILL


class hoist:
    """The context's switch for the sessions created inside; restored on exit (the context is shared by the whole run)."""

    def __init__(self, tsd_mod, gpu_ctx, on):
        self.lib, self.h, self.on = tsd_mod._lib.lib(), gpu_ctx.h, int(on)

    def __enter__(self):
        self.prev = self.lib.tsd_debug_set_session_hoist(self.h, self.on)
        assert self.prev in (0, 1)

    def __exit__(self, *exc):
        self.lib.tsd_debug_set_session_hoist(self.h, self.prev)


_REF = {}


def _lockstep(tsd_mod, model, sampler, cfg, on, req, k, pos, start=None):
    """Sample `pos` of a lockstep B = 3 session running request k there with its own cfg_scale: upload + set_seeds + seed_latents + steps
    0..3, or with `start` the img2img rule add_noise_seeded(start) + steps start..3 on the request's latents.  Computed once per case."""
    key = (sampler, cfg, on, k, pos, start)
    if key not in _REF:
        f = _filler()
        lat, ctx, uctx = f["lat"].copy(), f["ctx"].copy(), f["uctx"].copy()
        ctx[pos], uctx[pos] = req["ctx"], req["uctx"]
        if start is not None:
            lat[pos] = req["lat"]
        seeds = [91, 92, 93]
        seeds[pos] = req["seed"]
        s = tsd_mod.Session(model, None, B, L, T, cfg=cfg)
        s.set_sampler(*sampler)
        s.set_schedule(N_TRAIN, STEPS, 0)
        s.upload(lat, ctx, uctx if cfg else None, None, cfg_scale=req["scale"])
        s.set_seeds(seeds)
        if start is None:
            s.seed_latents()
        else:
            s.add_noise_seeded(start)
        for i in range(start or 0, STEPS):
            s.step(i)
        _REF[key] = s.latents()[pos].copy()
        s.close()
    return _REF[key]


def _open_slots(tsd_mod, model, sampler, cfg, nb=B):
    s = tsd_mod.Session(model, None, nb, L, T, cfg=cfg)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, STEPS, 0)
    s.slots_open()
    return s


def _start(s, b, req, cfg, **kw):
    s.slot_start(b, req["ctx"], req["uctx"] if cfg else None, seed=req["seed"], cfg_scale=req["scale"], **kw)


# ---- 1. staggered slots equal lockstep, bitwise -------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [1, 0], ids=["hoist", "nohoist"])
@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=IDS)
def test_staggered_slots_equal_lockstep_bitwise(gpu_ctx, tsd_mod, diffusion, sampler, cfg, on):
    """Request k starts in slot k after k advances, so from the second tick on every slot is at another index of the schedule; 6 ticks
    finish all three.  slot_latents(k) == sample k of the lockstep session of request k, bit for bit."""
    reqs = [_request(k) for k in range(B)]
    with hoist(tsd_mod, gpu_ctx, on):
        s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
        assert s.hoist_info()["active"] == on and s.slots_active() == 0
        for tick in range(6):
            if tick < B:
                _start(s, tick, reqs[tick], cfg)
                assert s.slot_state(tick) == (0, s.SLOT_ACTIVE)
            done = s.advance()
            assert done == ([tick - 3] if tick >= 3 else []), (tick, done)
        assert s.slots_active() == 0 and all(s.slot_state(k) == (STEPS, s.SLOT_DONE) for k in range(B))
        got = [s.slot_latents(k) for k in range(B)]
        s.close()
        for k in range(B):
            ref = _lockstep(tsd_mod, diffusion.model, sampler, cfg, on, reqs[k], k, k)
            assert np.isfinite(got[k]).all()
            assert np.array_equal(_bits(got[k]), _bits(ref)), (k, float(np.abs(got[k] - ref).max()))
    assert not np.array_equal(got[0], got[1])


# ---- 2. refill while others run --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", SAMPLERS, ids=IDS)
def test_a_finished_slot_is_refilled_while_the_others_run(gpu_ctx, tsd_mod, diffusion, sampler):
    """The staggered run of test 1 (CFG, hoist on); when slot 0 is done a fourth request - img2img: given latents, noised at the start,
    start_index 2 - takes it while slots 1 and 2 are mid-flight.  The refilled request equals add_noise_seeded(2) + steps 2, 3 of a
    lockstep session; slots 1 and 2 equal their references of test 1; the done slot reads the same bits until it is refilled."""
    cfg, on = True, 1
    reqs = [_request(k) for k in range(4)]
    with hoist(tsd_mod, gpu_ctx, on):
        s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
        got = {}
        for tick in range(6):
            if tick < B:
                _start(s, tick, reqs[tick], cfg)
            done = s.advance()
            if tick == 3:
                assert done == [0]
                first = s.slot_latents(0)
                assert s.slot_state(1) == (3, s.SLOT_ACTIVE) and s.slot_state(2) == (2, s.SLOT_ACTIVE)   # mid-flight
                again = s.slot_latents(0)
                _start(s, 0, reqs[3], cfg, latents=reqs[3]["lat"], noise_at_start=True, start_index=2)
                assert s.slot_state(0) == (2, s.SLOT_ACTIVE)
            for b in done:
                if tick != 3:
                    got[b] = s.slot_latents(b)
        assert sorted(got) == [0, 1, 2] and s.slots_active() == 0
        s.close()
        assert np.array_equal(_bits(first), _bits(again))
        assert np.array_equal(_bits(first), _bits(_lockstep(tsd_mod, diffusion.model, sampler, cfg, on, reqs[0], 0, 0)))
        refill = _lockstep(tsd_mod, diffusion.model, sampler, cfg, on, reqs[3], 3, 0, start=2)
        assert np.array_equal(_bits(got[0]), _bits(refill)), float(np.abs(got[0] - refill).max())
        for k in (1, 2):
            ref = _lockstep(tsd_mod, diffusion.model, sampler, cfg, on, reqs[k], k, k)
            assert np.array_equal(_bits(got[k]), _bits(ref)), (k, float(np.abs(got[k] - ref).max()))


# ---- 3. bystanders are not written --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [SAMPLERS[0], SAMPLERS[2]], ids=[IDS[0], IDS[2]])
def test_idle_and_done_slots_are_not_written(gpu_ctx, tsd_mod, diffusion, sampler):
    """Slot 0 starts at index 2 and is done after two advances, slot 1 runs on, slot 2 stays idle: over two further advances the done
    slot's and the idle slot's latents keep their bits (the raw device buffer, since an idle slot has nothing to download) while the
    active slot's change."""
    cfg = True
    reqs = [_request(k) for k in range(2)]
    s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
    _start(s, 0, reqs[0], cfg, latents=reqs[0]["lat"], noise_at_start=True, start_index=2)
    _start(s, 1, reqs[1], cfg)
    assert s.advance() == [] and s.advance() == [0]
    before, done_lat = s.raw_latents(), s.slot_latents(0)
    assert s.slot_state(2) == (0, s.SLOT_IDLE) and not before[2].any()   # zeroed by slots_open
    assert s.advance() == [] and s.advance() == [1]
    after = s.raw_latents()
    assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(_bits(after[2]), _bits(before[2]))
    assert np.array_equal(_bits(s.slot_latents(0)), _bits(done_lat))
    assert not np.array_equal(after[1], before[1]) and np.isfinite(after).all()
    s.close()


# ---- 4. launch accounting --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
def test_an_advance_makes_the_launches_of_a_seeded_step_plus_one(gpu_ctx, tsd_mod, diffusion, cfg):
    """Per-class launch counts over 2 ticks with the hoist on: an advance makes the launches of a seeded step() of the same shape plus
    exactly one elementwise launch (the gather of the per-sample time rows); and the hoisted buffers do not move over 8 advances."""
    P, sampler = 2, SAMPLERS[0]
    reqs = [_request(k) for k in range(B)]
    f = _filler()

    def counts(run_one, s):
        run_one(0)
        gpu_ctx.profile_begin()
        try:
            for i in range(1, 1 + P):
                run_one(i)
        finally:
            prof = gpu_ctx.profile_end()
        s.close()
        return {k: n for k, (_, n) in prof.items()}

    with hoist(tsd_mod, gpu_ctx, 1):
        a = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=cfg)
        a.set_sampler(*sampler)
        a.set_schedule(N_TRAIN, STEPS, 0)
        a.upload(f["lat"], f["ctx"], f["uctx"] if cfg else None, None)
        a.set_seeds([1, 2, 3])
        step = counts(a.step, a)
        b = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
        for k in range(B):
            _start(b, k, reqs[k], cfg)
        adv = counts(lambda i: b.advance(), b)
        want = dict(step, elementwise=step["elementwise"] + P)
        print(f"[slots] cfg={cfg}: launches per step {sum(step.values()) // P}, per advance {sum(adv.values()) // P}")
        assert adv == want, (adv, step)
        # the hoisted buffers are carved once: same addresses and size after 8 advances (two generations of requests)
        c = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
        info0 = c.hoist_info()
        assert info0["active"] == 1
        n = 0
        for gen in range(2):
            for k in range(B):
                _start(c, k, reqs[k], cfg)
            for _ in range(STEPS):
                c.advance()
                n += 1
        info1 = c.hoist_info()
        c.close()
        assert n == 8
        for key in ("time_table", "ctx_k", "ctx_vt", "bytes", "builds"):
            assert info1[key] == info0[key], (key, info0, info1)


# ---- 5. the state machine --------------------------------------------------------------------------------------------------------------
def test_state_machine(gpu_ctx, tsd_mod, diffusion):
    from tsd._lib import TSD_E_ARG, TSD_E_STATE, TSD_OK, ptr
    lib = tsd_mod._lib.lib()
    cfg, sampler = True, SAMPLERS[1]
    reqs = [_request(k) for k in range(B)]
    f = _filler()
    ctx0, uctx0 = np.ascontiguousarray(reqs[0]["ctx"], dtype=np.float32), np.ascontiguousarray(reqs[0]["uctx"], dtype=np.float32)
    buf = np.zeros((B, 4, L, L), dtype=np.float32)
    mask = C.c_uint32(0)
    s = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=cfg)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, STEPS, 0)
    # outside slot mode
    assert lib.tsd_session_advance(s.h, C.byref(mask)) == TSD_E_STATE
    assert lib.tsd_session_slot_start(s.h, 0, ptr(ctx0), ptr(uctx0), None, 0, 1, 0, 7.5) == TSD_E_STATE
    assert lib.tsd_session_slots_active(s.h) == 0
    s.slots_open()
    # no active slot; the lockstep entry points are closed
    assert lib.tsd_session_advance(s.h, C.byref(mask)) == TSD_E_STATE
    seeds = (C.c_uint64 * B)(1, 2, 3)
    m = np.ones((B, L, L), dtype=np.float32)
    assert lib.tsd_session_step(s.h, 0) == TSD_E_STATE and lib.tsd_session_set_seeds(s.h, seeds) == TSD_E_STATE
    assert lib.tsd_session_set_inpaint(s.h, ptr(m), ptr(buf), None) == TSD_E_STATE and lib.tsd_session_decode(s.h) == TSD_E_STATE
    assert lib.tsd_session_seed_latents(s.h) == TSD_E_STATE and lib.tsd_session_add_noise_seeded(s.h, 0) == TSD_E_STATE
    assert lib.tsd_session_add_noise(s.h, 0, ptr(buf)) == TSD_E_STATE and lib.tsd_session_download_latents(s.h, ptr(buf)) == TSD_E_STATE
    assert lib.tsd_session_slot_download(s.h, 0, ptr(buf)) == TSD_E_STATE   # idle
    # refusals of slot_start leave the slot as it was
    _start(s, 1, reqs[1], cfg)
    s.advance()
    state, lat = s.slot_state(1), s.slot_latents(1)
    assert state == (1, s.SLOT_ACTIVE)
    bad = ctx0.copy()
    bad[5, 7] = np.nan
    assert lib.tsd_session_slot_start(s.h, B, ptr(ctx0), ptr(uctx0), None, 0, 1, 0, 7.5) == TSD_E_ARG
    assert lib.tsd_session_slot_start(s.h, -1, ptr(ctx0), ptr(uctx0), None, 0, 1, 0, 7.5) == TSD_E_ARG
    assert lib.tsd_session_slot_start(s.h, 1, ptr(ctx0), ptr(uctx0), None, 0, 1, STEPS, 7.5) == TSD_E_ARG
    assert lib.tsd_session_slot_start(s.h, 1, ptr(bad), ptr(uctx0), None, 0, 1, 0, 7.5) == TSD_E_ARG
    assert lib.tsd_session_slot_start(s.h, 1, ptr(ctx0), None, None, 0, 1, 0, 7.5) == TSD_E_ARG   # CFG session without uncond
    assert lib.tsd_session_slot_start(s.h, 1, ptr(ctx0), ptr(uctx0), None, 0, 1, 0, float("inf")) == TSD_E_ARG
    assert s.slot_state(1) == state and np.array_equal(_bits(s.slot_latents(1)), _bits(lat)) and s.slots_active() == 1
    assert s.slot_state(0) == (0, s.SLOT_IDLE)
    # the refused calls left the request intact: it finishes on the bits of its lockstep reference
    for _ in range(STEPS - 1):
        done = s.advance()
    assert done == [1]
    assert np.array_equal(_bits(s.slot_latents(1)), _bits(_lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, reqs[1], 1, 1)))
    # upload() leaves slot mode; a lockstep run after it gives the bits of a fresh session
    s.upload(f["lat"], f["ctx"], f["uctx"], None, cfg_scale=7.5)
    assert lib.tsd_session_advance(s.h, C.byref(mask)) == TSD_E_STATE and lib.tsd_session_slots_active(s.h) == 0
    s.set_seeds([1, 2, 3])
    for i in range(STEPS):
        s.step(i)
    got = s.latents()
    s.close()
    fresh = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=cfg)
    fresh.set_sampler(*sampler)
    fresh.set_schedule(N_TRAIN, STEPS, 0)
    fresh.upload(f["lat"], f["ctx"], f["uctx"], None, cfg_scale=7.5)
    fresh.set_seeds([1, 2, 3])
    for i in range(STEPS):
        fresh.step(i)
    assert np.array_equal(_bits(got), _bits(fresh.latents()))
    # set_schedule leaves slot mode too
    fresh.slots_open()
    fresh.set_schedule(N_TRAIN, STEPS, 0)
    assert lib.tsd_session_advance(fresh.h, C.byref(mask)) == TSD_E_STATE
    fresh.close()
    assert lib.tsd_session_slots_open(None) == TSD_E_ARG and lib.tsd_session_slots_active(None) < 0 and TSD_OK == 0


@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
def test_parameters_set_between_two_advances_reach_the_next_advance(gpu_ctx, tsd_mod, cfg):
    """The rule of test_parameters_set_after_upload_reach_the_next_step, in slot mode: set_param of a k_proj weight and of a time-projection
    weight between two advances makes the next advance rebuild the hoisted buffers of all samples (a rebuild, not an error); the result is
    that of a slot session opened after the change - and differs from the old weights'."""
    own = tsd_mod.Diffusion(seed=SEED)   # this test changes parameters: a model of its own
    sampler = SAMPLERS[1]
    reqs = [_request(k) for k in range(B)]
    try:
        with hoist(tsd_mod, gpu_ctx, 1):
            s = _open_slots(tsd_mod, own.model, sampler, cfg)
            for k in range(B):
                _start(s, k, reqs[k], cfg)
            s.advance()
            before = [s.slot_latents(k) for k in range(B)]
            for k in range(B):   # the same requests again, from the start
                _start(s, k, reqs[k], cfg)
            builds = s.hoist_info()["builds"]
            specs = {name: (i, shape, bound) for i, (name, shape, _, bound) in enumerate(own.model.specs)}
            for k, name in enumerate((K_PROJ, T_PROJ)):
                i, shape, bound = specs[name]
                own.model.set_param(i, rng.uniform(SEED, 1590 + k, int(np.prod(shape)), bound).reshape(shape))
            s.advance()
            assert s.hoist_info()["builds"] == builds + 1
            first = [s.slot_latents(k) for k in range(B)]
            s.advance()
            assert s.hoist_info()["builds"] == builds + 1
            got = [s.slot_latents(k) for k in range(B)]
            s.close()
            fresh = _open_slots(tsd_mod, own.model, sampler, cfg)
            for k in range(B):
                _start(fresh, k, reqs[k], cfg)
            fresh.advance()
            fresh.advance()
            ref = [fresh.slot_latents(k) for k in range(B)]
            fresh.close()
        for k in range(B):
            assert np.isfinite(got[k]).all() and np.array_equal(_bits(got[k]), _bits(ref[k])), k
            assert not np.array_equal(first[k], before[k]), k   # the new weights change the result: a stale buffer would show
    finally:
        own.model.close()


# ---- 6. generate_stream ------------------------------------------------------------------------------------------------------------------
def test_generate_stream_gives_each_request_what_it_gives_alone(gpu_ctx, tsd_mod, diffusion):
    """Five txt2img requests through B = 2: five images, each equal to what `generate(..., seeds=...)` at B = 2 gives for the request in
    the sample position the scheduler put it in (greedy filling of equal-length requests: request k runs in slot k % 2)."""
    from tsd.serve import Request, generate_stream
    nb, steps = 2, 3
    dec = tsd_mod.Decoder(seed=SEED)
    reqs = [_request(k) for k in range(5)]
    stats = {}
    out = dict(generate_stream(diffusion, dec, (Request(k, r["ctx"], r["uctx"], r["seed"], r["scale"]) for k, r in enumerate(reqs)),
                               nb, L, T, cfg=True, inference_steps=steps, num_training_steps=N_TRAIN, stats=stats))
    assert sorted(out) == list(range(5))
    assert stats["advances"] == 3 * steps and stats["occupancy"] == 5 * steps / (nb * 3 * steps)
    f = _filler()
    for k, r in enumerate(reqs):
        pos = k % nb
        ctx, uctx = f["ctx"][:nb].copy(), f["uctx"][:nb].copy()
        ctx[pos], uctx[pos] = r["ctx"], r["uctx"]
        seeds = [5, 6]
        seeds[pos] = r["seed"]
        ref = tsd_mod.generate(diffusion, dec, ctx, uncond_context=uctx, cfg=True, cfg_scale=r["scale"], inference_steps=steps,
                               num_training_steps=N_TRAIN, L=L, seeds=seeds)
        img = out[k]
        assert img.shape == (3, 8 * L, 8 * L) and np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 255.0
        assert np.array_equal(_bits(img), _bits(ref[pos])), (k, float(np.abs(img - ref[pos]).max()))
    dec.model.close()
