"""GPU test of every per-request feature of the denoise session at once: seeded latents and step noise, seeded inpainting, guidance
rescale and a guidance scale per request, for the three samplers and both prediction types.  tests/test_gpu_slots.py,
test_gpu_slot_inpaint.py, test_gpu_guidance.py and test_gpu_vpred.py hold each feature on its own; step() and advance() assemble a step's
tables in one function, so the combination is held once: a slot's latents equal, bit for bit, the same sample of a lockstep session of
the same batch shape running the slot's request (lockstep takes one cfg_scale and one phi, so it runs once per request, the other sample
carrying filler).  Tiny-SD at random init (seed 1234), B = 2, L = 8, T = 77, 1000 training steps, 3 inference steps, CFG and hoist on."""
import numpy as np
import pytest

from oracle import rng

pytestmark = pytest.mark.gpu
SEED = 1234
N_TRAIN, STEPS = 1000, 3
B, L, T = 2, 8, 77
CHW = 4 * L * L
SCALES, PHIS = (7.5, 3.0), (0.7, 0.3)
# (prediction, zero_terminal_snr, sampler): epsilon on the spacings of tests/test_gpu_slots.py, v on trailing lists of the zero-terminal-SNR table
CASES = [("epsilon", False, ("ddpm", 0.0, "leading")), ("epsilon", False, ("ddim", 0.5, "trailing")),
         ("epsilon", False, ("dpmpp_2m", 0.0, "trailing")),
         ("v", True, ("ddpm", 0.0, "trailing")), ("v", True, ("ddim", 0.5, "trailing")), ("v", True, ("dpmpp_2m", 0.0, "trailing"))]
IDS = [f"{p}-{s[0]}" for p, _, s in CASES]


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mask(k):
    """Mask k (L,L): v = (cell * (2k + 3) + k) mod 13 -> 0 below 4, 1 above 9, v / 16 between."""
    cell = np.arange(L * L).reshape(L, L)
    v = (cell * (2 * k + 3) + k) % 13
    return np.where(v < 4, 0.0, np.where(v > 9, 1.0, v / 16.0)).astype(np.float32)


def _request(k):
    """Request k: its own context, uncond context, seed (the latents and all noise come from it), guidance scale, rescale phi, mask and
    known latents."""
    return dict(ctx=rng.normal(SEED, 1900 + 10 * k, T * 768).reshape(T, 768), uctx=rng.normal(SEED, 1901 + 10 * k, T * 768).reshape(T, 768),
                seed=3000017 * (k + 1) + 31, scale=SCALES[k], phi=PHIS[k], mask=_mask(k),
                known=rng.normal(SEED, 1902 + 10 * k, CHW).reshape(4, L, L).astype(np.float32))


def _configure(s, pred, ztsnr, sampler):
    s.set_prediction(pred, ztsnr)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, STEPS, 0)


def _lockstep(tsd_mod, model, pred, ztsnr, sampler, req, pos):
    """Sample `pos` of a lockstep session running `req` there - upload, set_seeds, seed_latents, set_inpaint(seeded), set_guidance_rescale,
    steps 0..2 - with finite filler (an all-ones mask, another seed) in the other sample."""
    lat = rng.normal(SEED, 1890, B * CHW).reshape(B, 4, L, L).astype(np.float32)
    ctx, uctx = rng.normal(SEED, 1891, B * T * 768).reshape(B, T, 768), rng.normal(SEED, 1892, B * T * 768).reshape(B, T, 768)
    masks, seeds = np.ones((B, L, L), dtype=np.float32), [91, 92]
    ctx[pos], uctx[pos], masks[pos], seeds[pos] = req["ctx"], req["uctx"], req["mask"], req["seed"]
    known = lat.copy()
    known[pos] = req["known"]
    s = tsd_mod.Session(model, None, B, L, T, cfg=True)
    _configure(s, pred, ztsnr, sampler)
    s.upload(lat, ctx, uctx, None, cfg_scale=req["scale"])
    s.set_seeds(seeds)
    s.seed_latents()
    s.set_inpaint(masks, known, seeded=True)
    s.set_guidance_rescale(req["phi"])
    for i in range(STEPS):
        s.step(i)
    out = s.latents()[pos].copy()
    s.close()
    return out


@pytest.mark.parametrize("pred,ztsnr,sampler", CASES, ids=IDS)
def test_slots_with_every_feature_equal_lockstep_bitwise(gpu_ctx, tsd_mod, diffusion, pred, ztsnr, sampler):
    """Both requests start together, each with its own seed, guidance scale, mask and phi; after three advances slot_latents(k) == sample
    k of request k's lockstep run as uint32 bit patterns, everything is finite and the two requests differ."""
    lib = tsd_mod._lib.lib()
    reqs = [_request(k) for k in range(B)]
    for m in (r["mask"] for r in reqs):
        assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
    assert not np.array_equal(reqs[0]["mask"], reqs[1]["mask"])
    prev = lib.tsd_debug_set_session_hoist(gpu_ctx.h, 1)
    assert prev in (0, 1)
    try:
        s = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=True)
        _configure(s, pred, ztsnr, sampler)
        s.slots_open()
        assert s.hoist_info()["active"] == 1
        for k, r in enumerate(reqs):
            s.slot_start(k, r["ctx"], r["uctx"], seed=r["seed"], cfg_scale=r["scale"])
            s.slot_set_inpaint(k, r["mask"], r["known"])
            s.slot_set_guidance_rescale(k, r["phi"])
        done = [s.advance() for _ in range(STEPS)]
        assert done == [[], [], [0, 1]], done
        got = [s.slot_latents(k) for k in range(B)]
        s.close()
        refs = [_lockstep(tsd_mod, diffusion.model, pred, ztsnr, sampler, reqs[k], k) for k in range(B)]
    finally:
        lib.tsd_debug_set_session_hoist(gpu_ctx.h, prev)
    for k in range(B):
        assert np.isfinite(got[k]).all() and np.isfinite(refs[k]).all(), k
        assert np.array_equal(_bits(got[k]), _bits(refs[k])), (k, float(np.abs(got[k] - refs[k]).max()))
    assert not np.array_equal(got[0], got[1])
