"""GPU tests of inpainting in slot sessions: `Session.slot_set_inpaint` and the update launch that blends (k_slot_update_blend).  The
reference is always the lockstep path - upload + set_seeds + add_noise_seeded + set_inpaint(seeded) + step, which tests/test_gpu_inpaint.py
holds to float64 - in a session of the same batch shape with the request in the same sample position, so every comparison is bitwise.
Tiny-SD at random init (seed 1234), B = 3, L = 8, T = 77, 1000 training steps, 4 inference steps (the shape of tests/test_gpu_slots.py).
The masks differ per request, are not symmetric under transposition, hold 0, 1 and fractions and have distinct rows: a swapped axis, a
wrong channel stride or another slot's mask changes bits."""
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
IDS = ["ddpm", "ddim", "dpmpp_2m", "ddpm_trailing"]
SCALES = (7.5, 3.0, 1.0)
ONES = np.ones((L, L), dtype=np.float32)


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _request(k):
    """Request k: its own context, uncond context, seed, guidance scale and latents (the known latents of an inpainting request)."""
    return dict(ctx=rng.normal(SEED, 1700 + 10 * k, T * 768).reshape(T, 768), uctx=rng.normal(SEED, 1701 + 10 * k, T * 768).reshape(T, 768),
                seed=2000003 * (k + 1) + 29, scale=SCALES[k % 3], lat=rng.normal(SEED, 1702 + 10 * k, CHW).reshape(4, L, L).astype(np.float32))


def _mask(k):
    """Mask k (L,L): v = (cell * (2k + 3) + k) mod 13 -> 0 below 4, 1 above 9, v / 16 between."""
    cell = np.arange(L * L).reshape(L, L)
    v = (cell * (2 * k + 3) + k) % 13
    return np.where(v < 4, 0.0, np.where(v > 9, 1.0, v / 16.0)).astype(np.float32)


def test_the_masks_can_tell_the_mistakes_apart():
    ms = [_mask(k) for k in range(4)]
    for k, m in enumerate(ms):
        assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
        assert not np.array_equal(m, m.T)
        assert len({r.tobytes() for r in m}) == L
        assert all(not np.array_equal(m, o) for o in ms[:k])


_FILL = {}


def _filler():
    """Finite data for the other samples of a lockstep reference (made once)."""
    if not _FILL:
        _FILL["lat"] = rng.normal(SEED, 1690, B * CHW).reshape(B, 4, L, L).astype(np.float32)
        _FILL["ctx"] = rng.normal(SEED, 1691, B * T * 768).reshape(B, T, 768)
        _FILL["uctx"] = rng.normal(SEED, 1692, B * T * 768).reshape(B, T, 768)
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


def _lockstep(tsd_mod, model, sampler, cfg, on, k, pos, start, mask_k=None, off_after=None, nb=B, steps=STEPS):
    """Sample `pos` of a lockstep session of nb samples running request k there, img2img from index `start`: upload, set_seeds,
    add_noise_seeded(start), with mask_k set_inpaint(seeded) - mask k for this sample, all ones for the others - then step start..  With
    off_after = i, set_inpaint(None) follows step i.  Computed once per case, never changed."""
    key = (sampler, cfg, on, k, pos, start, mask_k, off_after, nb, steps)
    if key not in _REF:
        f, req = _filler(), _request(k)
        lat, ctx, uctx = f["lat"][:nb].copy(), f["ctx"][:nb].copy(), f["uctx"][:nb].copy()
        lat[pos], ctx[pos], uctx[pos] = req["lat"], req["ctx"], req["uctx"]
        seeds = [91, 92, 93][:nb]
        seeds[pos] = req["seed"]
        s = tsd_mod.Session(model, None, nb, L, T, cfg=cfg)
        s.set_sampler(*sampler)
        s.set_schedule(N_TRAIN, steps, 0)
        s.upload(lat, ctx, uctx if cfg else None, None, cfg_scale=req["scale"])
        s.set_seeds(seeds)
        s.add_noise_seeded(start)
        if mask_k is not None:
            masks = np.ones((nb, L, L), dtype=np.float32)
            masks[pos] = _mask(mask_k)
            s.set_inpaint(masks, lat, seeded=True)
        for i in range(start, steps):
            s.step(i)
            if off_after == i:
                s.set_inpaint(None)
        _REF[key] = s.latents()[pos].copy()
        s.close()
    return _REF[key]


def _open_slots(tsd_mod, model, sampler, cfg, nb=B, steps=STEPS):
    s = tsd_mod.Session(model, None, nb, L, T, cfg=cfg)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, steps, 0)
    s.slots_open()
    return s


def _start(s, b, k, cfg, start, mask=None):
    """Request k as img2img from index `start` in slot b; with `mask` (an (L,L) array) as an inpainting request."""
    req = _request(k)
    s.slot_start(b, req["ctx"], req["uctx"] if cfg else None, latents=req["lat"], noise_at_start=True, seed=req["seed"],
                 start_index=start, cfg_scale=req["scale"])
    assert not s.slot_inpaint_active(b)
    if mask is not None:
        s.slot_set_inpaint(b, mask, req["lat"])
        assert s.slot_inpaint_active(b)


# ---- 1. staggered slots equal lockstep, bitwise -------------------------------------------------------------------------------------
CASES = [(sm, cfg, 1) for sm in SAMPLERS for cfg in (False, True)] + [(SAMPLERS[0], True, 0)]
CASE_IDS = [f"{IDS[SAMPLERS.index(sm)]}-{'cfg' if cfg else 'nocfg'}-{'hoist' if on else 'nohoist'}" for sm, cfg, on in CASES]


@pytest.mark.parametrize("sampler,cfg,on", CASES, ids=CASE_IDS)
def test_staggered_inpainting_slots_equal_lockstep_bitwise(gpu_ctx, tsd_mod, diffusion, sampler, cfg, on):
    """Slot 0: inpainting from index 0 (mask 0).  Slot 1: plain img2img from index 1.  Slot 2: inpainting from index 2 (mask 2).  They start on
    successive ticks, so every advance from the second on blends slots at different timesteps next to one that does not blend; all finish at
    the fourth.  Each slot's latents == the same sample of the lockstep session of its request, bit for bit."""
    plan = [(0, 0, 0), (1, 1, None), (2, 2, 2)]   # (slot = request, start index, mask)
    with hoist(tsd_mod, gpu_ctx, on):
        s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
        assert s.hoist_info()["active"] == on
        for tick in range(4):
            if tick < B:
                k, start, mk = plan[tick]
                _start(s, k, k, cfg, start, None if mk is None else _mask(mk))
            done = s.advance()
            assert done == ([0, 1, 2] if tick == 3 else []), (tick, done)
        got = [s.slot_latents(k) for k in range(B)]
        assert not any(s.slot_inpaint_active(k) for k in range(B))   # a done slot reports none
        s.close()
        for k, start, mk in plan:
            ref = _lockstep(tsd_mod, diffusion.model, sampler, cfg, on, k, k, start, mk)
            assert np.isfinite(got[k]).all()
            assert _same(got[k], ref), (k, float(np.abs(got[k] - ref).max()))
        # the mask matters: without it slot 0 ends elsewhere
        assert not _same(got[0], _lockstep(tsd_mod, diffusion.model, sampler, cfg, on, 0, 0, 0, None))


# ---- 2. exact ends ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [SAMPLERS[0], SAMPLERS[2]], ids=[IDS[0], IDS[2]])
def test_exact_ends(gpu_ctx, tsd_mod, diffusion, sampler):
    """Slot 0 with an all-ones mask gives the bits of the same request without inpainting (run next in the same slot); slot 1 with an
    all-zeros mask ends on its known latents bit for bit (the last step's blend is 1 * known + 0 * noise)."""
    cfg = True
    s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
    _start(s, 0, 0, cfg, 1, ONES)
    _start(s, 1, 1, cfg, 0, np.zeros((L, L), dtype=np.float32))
    for _ in range(STEPS):
        s.advance()
    ones, zeros = s.slot_latents(0), s.slot_latents(1)
    _start(s, 0, 0, cfg, 1)
    for _ in range(STEPS - 1):
        s.advance()
    plain = s.slot_latents(0)
    s.close()
    assert np.isfinite(ones).all() and _same(ones, plain)
    assert _same(ones, _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 0, 0, 1, None))
    assert _same(zeros, _request(1)["lat"])


# ---- 3. no stale state ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [SAMPLERS[0], SAMPLERS[2]], ids=[IDS[0], IDS[2]])
def test_a_refilled_slot_does_not_inherit_the_mask(gpu_ctx, tsd_mod, diffusion, sampler):
    """Slot 0 runs an inpainting request; a plain img2img request then takes the slot - once mid-flight, once after it is done - and equals
    its lockstep reference without a mask."""
    cfg = True
    s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
    _start(s, 0, 0, cfg, 0, _mask(0))
    s.advance()
    assert s.slot_inpaint_active(0)
    _start(s, 0, 1, cfg, 2)                      # replaces the active inpainting request
    assert not s.slot_inpaint_active(0)
    assert s.advance() == [] and s.advance() == [0]
    mid = s.slot_latents(0)
    _start(s, 0, 0, cfg, 0, _mask(0))
    for _ in range(STEPS):
        s.advance()
    assert s.slot_state(0) == (STEPS, s.SLOT_DONE)
    _start(s, 0, 3, cfg, 1)                      # takes the done slot
    for _ in range(STEPS - 1):
        s.advance()
    after = s.slot_latents(0)
    s.close()
    assert _same(mid, _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 1, 0, 2, None))
    assert _same(after, _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 3, 0, 1, None))


@pytest.mark.parametrize("sampler", [SAMPLERS[0], SAMPLERS[2]], ids=[IDS[0], IDS[2]])
def test_turning_the_mask_off_mid_flight_equals_lockstep(gpu_ctx, tsd_mod, diffusion, sampler):
    """slot_set_inpaint(b, None) after the slot's second step == the lockstep session that calls set_inpaint(None) after step 1 (the
    history is dropped in both: step 2 of DPM-Solver++(2M) is first order); the neighbour slot keeps its mask throughout."""
    cfg = True
    s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
    _start(s, 1, 1, cfg, 0, _mask(1))
    _start(s, 2, 2, cfg, 0, _mask(2))
    s.advance()
    s.advance()
    s.slot_set_inpaint(1, None)
    assert not s.slot_inpaint_active(1) and s.slot_inpaint_active(2)
    s.advance()
    assert s.advance() == [1, 2]
    got1, got2 = s.slot_latents(1), s.slot_latents(2)
    s.close()
    assert _same(got1, _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 1, 1, 0, 1, off_after=1))
    assert not _same(got1, _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 1, 1, 0, 1))
    assert _same(got2, _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 2, 2, 0, 2))


def test_idle_and_done_slots_are_not_written_by_a_blending_advance(gpu_ctx, tsd_mod, diffusion):
    """Slot 0 (inpainting from index 2) is done after two advances, slot 1 (inpainting from 0) runs on, slot 2 stays idle: over the two
    further advances, which blend slot 1, the done and the idle slot's raw latents keep their bits."""
    cfg, sampler = True, SAMPLERS[0]
    s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
    _start(s, 0, 0, cfg, 2, _mask(0))
    _start(s, 1, 1, cfg, 0, _mask(1))
    assert s.advance() == [] and s.advance() == [0]
    before = s.raw_latents()
    assert s.slot_state(2) == (0, s.SLOT_IDLE) and not before[2].any()
    assert s.slot_inpaint_active(1) and not s.slot_inpaint_active(0)
    assert s.advance() == [] and s.advance() == [1]
    after = s.raw_latents()
    s.close()
    assert _same(after[0], before[0]) and _same(after[2], before[2])
    assert not _same(after[1], before[1]) and np.isfinite(after).all()
    assert _same(after[0], _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 0, 0, 2, 0))
    assert _same(after[1], _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 1, 1, 0, 1))


# ---- 4. launch accounting --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
def test_an_advance_with_inpainting_makes_the_launches_of_one_without(gpu_ctx, tsd_mod, diffusion, cfg):
    """Per-class launch counts of tsd_ctx_profile_begin / _end over 2 advances (hoist on, all three slots active): with two inpainting
    slots exactly the counts without any.  (The profile counts launches; that no advance copies from the host is what
    tests/test_slot_inpaint_cpu.py reads off the entry point's text.)"""
    P, sampler = 2, SAMPLERS[0]

    def counts(masked):
        s = _open_slots(tsd_mod, diffusion.model, sampler, cfg)
        for k in range(B):
            _start(s, k, k, cfg, 0, _mask(k) if k in masked else None)
        s.advance()
        gpu_ctx.profile_begin()
        try:
            for _ in range(P):
                s.advance()
        finally:
            prof = gpu_ctx.profile_end()
        s.close()
        return {k: n for k, (_, n) in prof.items()}

    with hoist(tsd_mod, gpu_ctx, 1):
        plain, blend = counts(()), counts((0, 2))
    print(f"[slot inpaint] cfg={cfg}: launches per advance {sum(plain.values()) // P} without, {sum(blend.values()) // P} with inpainting slots")
    assert sum(plain.values()) > 0 and blend == plain, (blend, plain)


# ---- 5. refusals and state ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_slot_as_it_was(gpu_ctx, tsd_mod, diffusion):
    from tsd._lib import TSD_E_ARG, TSD_E_STATE, TSD_OK, ptr
    lib = tsd_mod._lib.lib()
    cfg, sampler = True, SAMPLERS[1]
    f = _filler()
    mask, known = _mask(3), np.ascontiguousarray(_request(1)["lat"])
    s = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=cfg)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, STEPS, 0)
    # outside slot mode: before slots_open, and in a lockstep upload
    assert lib.tsd_session_slot_set_inpaint(s.h, 0, ptr(mask), ptr(known)) == TSD_E_STATE
    assert lib.tsd_session_slot_inpaint_active(s.h, 0) == TSD_E_STATE
    s.upload(f["lat"], f["ctx"], f["uctx"], None)
    assert lib.tsd_session_slot_set_inpaint(s.h, 0, ptr(mask), ptr(known)) == TSD_E_STATE
    assert lib.tsd_session_slot_set_inpaint(None, 0, ptr(mask), ptr(known)) == TSD_E_ARG and lib.tsd_session_slot_inpaint_active(None, 0) == TSD_E_ARG
    s.slots_open()
    # slot 0: done (inpainting from index 3, one advance); slot 1: active with mask 1, one step in; slot 2: idle
    _start(s, 0, 0, cfg, 3, _mask(0))
    _start(s, 1, 1, cfg, 0, _mask(1))
    assert s.advance() == [0]

    def snapshot():
        return s.raw_latents(), [s.slot_state(b) for b in range(B)], [s.slot_inpaint_active(b) for b in range(B)]

    lat0, st0, ip0 = snapshot()
    assert st0 == [(STEPS, s.SLOT_DONE), (1, s.SLOT_ACTIVE), (0, s.SLOT_IDLE)] and ip0 == [False, True, False]

    def refused(code, *args):
        assert lib.tsd_session_slot_set_inpaint(s.h, *args) == code, args[0]
        lat, st, ip = snapshot()
        assert _same(lat, lat0) and st == st0 and ip == ip0

    refused(TSD_E_ARG, -1, ptr(mask), ptr(known))
    refused(TSD_E_ARG, B, ptr(mask), ptr(known))
    for v in (np.nan, np.inf, -0.25, 1.5):
        bad = mask.copy()
        bad[L - 1, L - 2] = v                      # late in the mask: the refusal still comes before the first copy
        refused(TSD_E_ARG, 1, ptr(bad), ptr(known))
    refused(TSD_E_ARG, 1, ptr(mask), None)
    for v in (np.nan, -np.inf):
        bad = known.copy()
        bad[3, L - 1, L - 1] = v
        refused(TSD_E_ARG, 1, ptr(mask), ptr(bad))
    refused(TSD_E_STATE, 0, ptr(mask), ptr(known))   # done
    refused(TSD_E_STATE, 2, ptr(mask), ptr(known))   # idle
    refused(TSD_E_STATE, 0, None, None)              # turning it off is refused there as well
    refused(TSD_E_STATE, 2, None, None)
    assert lib.tsd_session_slot_inpaint_active(s.h, -1) == TSD_E_ARG and lib.tsd_session_slot_inpaint_active(s.h, B) == TSD_E_ARG
    # the lockstep calls stay refused in slot mode
    m3, k3 = np.ones((B, L, L), dtype=np.float32), np.zeros((B, 4, L, L), dtype=np.float32)
    assert lib.tsd_session_set_inpaint(s.h, ptr(m3), ptr(k3), None) == TSD_E_STATE
    assert lib.tsd_session_set_inpaint_seeded(s.h, ptr(m3), ptr(k3)) == TSD_E_STATE
    # the refused calls wrote nothing: slot 1 finishes on the bits of its lockstep reference (its own mask and known latents)
    for _ in range(STEPS - 1):
        done = s.advance()
    assert done == [1]
    assert _same(s.slot_latents(1), _lockstep(tsd_mod, diffusion.model, sampler, cfg, 1, 1, 1, 0, 1))
    # slots_open turns every slot's inpainting off; the Python layer checks shapes before the library is called
    _start(s, 1, 1, cfg, 0, _mask(1))
    s.slots_open()
    assert [lib.tsd_session_slot_inpaint_active(s.h, b) for b in range(B)] == [0, 0, 0]
    _start(s, 1, 1, cfg, 0)
    for args in ((np.ones((L, L + 1)), known), (mask, None), (mask, np.zeros((3, L, L))), (np.ones((2, L, L)), known)):
        with pytest.raises(ValueError):
            s.slot_set_inpaint(1, *args)
    s.slot_set_inpaint(1, mask[None], known[None])   # (1,L,L) and (1,4,L,L) are accepted
    assert s.slot_inpaint_active(1) and lib.tsd_session_slot_set_inpaint(s.h, 1, None, None) == TSD_OK and not s.slot_inpaint_active(1)
    s.close()


# ---- 6. generate_stream ------------------------------------------------------------------------------------------------------------------
def test_generate_stream_inpaints_mask_requests_in_their_slots(gpu_ctx, tsd_mod, diffusion):
    """A queue of txt2img, img2img and mask requests through B = 2 (latents returned, no decoder).  Greedy filling puts request 0 (txt2img)
    and 1 (latent mask, strength 1) into slots 0 and 1; both finish after 4 advances, then 2 (img2img, strength 0.5) and 3 (pixel mask,
    strength 0.5) take slots 0 and 1, and 4 (latent mask (1,L,L), strength 0.75) takes whichever ends first: slot 0.  Every mask request
    equals the manual slot calls for it in the same sample position."""
    from tsd.serve import Request, generate_stream, start_index
    nb = 2
    reqs = [_request(k) for k in range(5)]
    px = np.zeros((8 * L, 8 * L), dtype=np.float32)
    px[5:29, 11:50] = 1.0
    px[40:44, 0:9] = 0.75
    queue = [Request(0, reqs[0]["ctx"], reqs[0]["uctx"], reqs[0]["seed"], reqs[0]["scale"]),
             Request(1, reqs[1]["ctx"], reqs[1]["uctx"], reqs[1]["seed"], reqs[1]["scale"], reqs[1]["lat"], 1.0, _mask(1)),
             Request(2, reqs[2]["ctx"], reqs[2]["uctx"], reqs[2]["seed"], reqs[2]["scale"], reqs[2]["lat"], 0.5),
             Request(3, reqs[3]["ctx"], reqs[3]["uctx"], reqs[3]["seed"], reqs[3]["scale"], reqs[3]["lat"], 0.5, mask=px[None], mask_mode="any"),
             Request(4, reqs[4]["ctx"], reqs[4]["uctx"], reqs[4]["seed"], reqs[4]["scale"], reqs[4]["lat"], 0.75, _mask(0)[None])]
    stats = {}
    out = dict(generate_stream(diffusion, None, iter(queue), nb, L, T, cfg=True, inference_steps=STEPS, num_training_steps=N_TRAIN,
                               return_latents=True, stats=stats))
    assert sorted(out) == list(range(5)) and stats["advances"] == 4 + 2 + 3
    lat_px = tsd_mod.utils.latent_mask(px[None], "any")[0]
    assert lat_px.shape == (L, L) and 0 < lat_px.sum() < L * L
    for k, pos, mask in ((1, 1, _mask(1)), (3, 1, lat_px), (4, 0, _mask(0))):
        r = queue[k]
        i0 = start_index(STEPS, r.strength)
        s = _open_slots(tsd_mod, diffusion.model, SAMPLERS[0], True, nb=nb)
        s.slot_start(pos, r.context, r.uncond, latents=r.latents, noise_at_start=True, seed=r.seed, start_index=i0, cfg_scale=r.cfg_scale)
        s.slot_set_inpaint(pos, mask, r.latents)
        for _ in range(STEPS - i0):
            done = s.advance()
        assert done == [pos]
        ref = s.slot_latents(pos)
        s.close()
        assert np.isfinite(out[k]).all() and _same(out[k], ref), (k, float(np.abs(out[k] - ref).max()))
    # the latent-mask request is also what the lockstep path gives for it at this batch shape
    assert _same(out[1], _lockstep(tsd_mod, diffusion.model, SAMPLERS[0], True, 1, 1, 1, 0, 1, nb=nb))
    with pytest.raises(ValueError):   # a mask without latents: refused before any slot is touched
        list(generate_stream(diffusion, None, iter([Request(9, reqs[0]["ctx"], reqs[0]["uctx"], 1, 7.5, None, None, _mask(0))]), nb, L, T,
                             cfg=True, inference_steps=STEPS, num_training_steps=N_TRAIN, return_latents=True))
