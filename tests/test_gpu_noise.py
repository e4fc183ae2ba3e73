"""GPU tests of the seeded device-side noise: `tsd_normal_fill_f32` against the float64 twin with a derived error bound, a seeded
session against the same session fed the device's own stream (bitwise), the seeded latents / add_noise / inpainting entries against
their host-tensor counterparts (bitwise), batch invariance, launch accounting, the state machine and `generate(seeds=...)`."""
import ctypes as C

import numpy as np
import pytest

import noise_ref
from noise_ref import M64, STREAM_ADD_NOISE, STREAM_LATENTS, STREAM_STEP0
from oracle import rng
from sampler_ref import N_TRAIN

pytestmark = pytest.mark.gpu
SEED = 1234
L, T = 8, 77
CHW = 4 * L * L
SAMPLERS = [("ddpm", 0.0, "leading"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")]
# |z_dev - z_twin| <= EPS * max(|z_twin|, 2^-20).  Derived above normal_counter (csrc/counter_rng.h) from the per-operation bounds: log 3 ulp
# (halved by the root), an exact * (-2), a correctly rounded sqrt 0.5 ulp, cospi of an exact argument 4 ulp, one product 0.5 ulp, the
# twin's rounding to float32 0.5 ulp = 7 ulp = 14 * 2^-24; the condition of the issue is EPS <= 16 * 2^-24.
EPS = 14 * 2.0 ** -24
assert EPS <= 16 * 2.0 ** -24


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _inputs(B, tag=1300):
    lat, known = (rng.normal(SEED, tag + k, B * CHW).reshape(B, 4, L, L) for k in (0, 3))
    ctx, uctx = (rng.normal(SEED, tag + k, B * T * 768).reshape(B, T, 768) for k in (1, 2))
    return lat, ctx, uctx, known


def _open(tsd_mod, model, B, sampler, cfg, steps, lat, ctx, uctx, noise=None, start=0):
    s = tsd_mod.Session(model, None, B, L, T, cfg=cfg)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, steps, start)
    s.upload(lat, ctx, uctx if cfg else None, noise, cfg_scale=7.5)
    return s


def _stream(tsd_mod, ctx, seeds, stream):
    """[B,4,L,L]: sample b is the device's own stream (seeds[b], stream), counters 0 .. 4 L^2 - 1"""
    return np.stack([tsd_mod.normal_fill(s, stream, CHW, 0, ctx) for s in seeds]).reshape(len(seeds), 4, L, L)


def _step_noise(tsd_mod, ctx, seeds, steps):
    return np.stack([_stream(tsd_mod, ctx, seeds, STREAM_STEP0 + i) for i in range(steps)])


def _mask(B):
    m = np.zeros((B, L, L), dtype=np.float32)
    m[:, :, : L // 2 - 1] = 1.0
    m[:, :, L // 2 - 1] = 0.75
    m[:, :, L // 2] = 0.3
    return m


# ---- 5. the fill kernel against the twin ----------------------------------------------------------------------------------------------
def test_normal_fill_matches_the_twin_within_the_derived_bound(gpu_ctx, tsd_mod):
    """n = 70068 (no multiple of the 256-thread block) at offsets 0, 12345 and 2^33 + 5 (the counter does not fit 32 bits) with seeds 0 and
    2^64 - 1: finite, |z| <= 5.78, |z_dev - z_twin| <= EPS max(|z_twin|, 2^-20) with EPS = 14 * 2^-24 (derived, see EPS above), and a fill
    split at an arbitrary offset gives the bits of the whole fill.
    Measured on an MI355X over exactly these inputs: worst |z_dev - z_twin| / max(|z_twin|, 2^-20) = 3.99 * 2^-24."""
    n, stream = 70068, 16
    worst = 0.0
    for seed in (0, M64):
        for off in (0, 12345, (1 << 33) + 5):
            got = tsd_mod.normal_fill(seed, stream, n, off, gpu_ctx)
            twin = tsd_mod.rng.normal_counter(seed, stream, n, offset=off)
            assert got.dtype == np.float32 and got.shape == (n,)
            assert np.isfinite(got).all() and np.abs(got).max() <= 5.78
            ratio = np.abs(got.astype(np.float64) - twin) / np.maximum(np.abs(twin.astype(np.float64)), 2.0 ** -20)
            worst = max(worst, float(ratio.max()))
            print(f"[noise] fill seed={seed:#x} offset={off}: worst error / max(|z|, 2^-20) = {ratio.max() * 2 ** 24:.2f} * 2^-24, "
                  f"bitwise equal to the twin in {np.mean(_bits(got) == _bits(twin)) * 100:.1f} %")
            assert ratio.max() <= EPS, (seed, off, float(ratio.max()) * 2 ** 24)
            cut = 31337
            parts = np.concatenate([tsd_mod.normal_fill(seed, stream, cut, off, gpu_ctx),
                                    tsd_mod.normal_fill(seed, stream, n - cut, off + cut, gpu_ctx)])
            assert np.array_equal(_bits(parts), _bits(got)), (seed, off)
    print(f"[noise] fill: measured maximum {worst * 2 ** 24:.2f} * 2^-24, bound {EPS * 2 ** 24:.0f} * 2^-24")
    # the known answers of the issue, through the device, within the same bound
    for seed, stream, j, _, _, bits in noise_ref.KNOWN_ANSWERS:
        want = np.array([bits], dtype=np.uint32).view(np.float32)[0]
        z = tsd_mod.normal_fill(seed, stream, 1, j, gpu_ctx)[0]
        assert abs(float(z) - float(want)) <= EPS * max(abs(float(want)), 2.0 ** -20), (seed, stream, j, z, want)


def test_moments_of_one_device_fill(gpu_ctx, tsd_mod):
    """The moment checks of tests/test_noise_cpu.py on 2^20 values drawn by the device (bound 5 each)."""
    n = 1 << 20
    z = tsd_mod.normal_fill(12345, 2, n, 0, gpu_ctx)
    z_next = tsd_mod.normal_fill(12346, 2, n, 0, gpu_ctx)
    sc = noise_ref.moment_scores(z, z_next)
    print("[noise] device fill: " + " ".join(f"{k}={v:.2f}" for k, v in sc.items()))
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.78
    for k in ("mean", "var", "m3", "m4", "lag1", "next_seed"):
        assert sc[k] <= 5.0, (k, sc[k])


# ---- 6. a seeded session against the same session fed the device's own stream ------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=lambda s: s[0])
def test_seeded_steps_equal_steps_on_the_uploaded_stream_bitwise(gpu_ctx, tsd_mod, diffusion, sampler, cfg):
    """upload(noise=None) + set_seeds, 4 steps == upload(noise[i, b] = normal_fill(seeds[b], 16 + i, 0, 4 L^2)), 4 steps, bitwise: the
    inline draw of the update kernels is the fill kernel's function, and the update around it rounds as it did."""
    B, steps = 2, 4
    seeds = [7, M64 - 3]
    lat, ctx, uctx, _ = _inputs(B)
    a = _open(tsd_mod, diffusion.model, B, sampler, cfg, steps, lat, ctx, uctx, None)
    a.set_seeds(seeds)
    assert a.seeds_active
    b = _open(tsd_mod, diffusion.model, B, sampler, cfg, steps, lat, ctx, uctx, _step_noise(tsd_mod, gpu_ctx, seeds, steps))
    c = _open(tsd_mod, diffusion.model, B, sampler, cfg, steps, lat, ctx, uctx, None)   # noiseless
    for i in range(steps):
        for s in (a, b, c):
            s.step(i)
        la, lb = a.latents(), b.latents()
        assert np.isfinite(la).all()
        assert np.array_equal(_bits(la), _bits(lb)), (sampler[0], cfg, i, float(np.abs(la - lb).max()))
    lc = c.latents()
    if sampler[0] == "dpmpp_2m":
        assert np.array_equal(_bits(la), _bits(lc))   # takes no noise: the seeds change nothing
    else:
        assert not np.array_equal(la, lc)              # and elsewhere the noise is really there
    for s in (a, b, c):
        s.close()


# ---- 7. the seeded entries against their host-tensor counterparts --------------------------------------------------------------------------
def test_seed_latents_add_noise_and_inpaint_equal_their_host_tensor_counterparts_bitwise(gpu_ctx, tsd_mod, diffusion):
    B, steps = 2, 4
    seeds = [11, (1 << 63) + 7]
    sampler = SAMPLERS[0]
    lat, ctx, uctx, known = _inputs(B, tag=1310)
    z2, z4 = _stream(tsd_mod, gpu_ctx, seeds, STREAM_LATENTS), _stream(tsd_mod, gpu_ctx, seeds, STREAM_ADD_NOISE)
    noise = _step_noise(tsd_mod, gpu_ctx, seeds, steps)
    # seed_latents: the latents are stream 2, and the steps that follow are those of a session that uploaded them
    a = _open(tsd_mod, diffusion.model, B, sampler, False, steps, np.zeros_like(lat), ctx, uctx, None)
    a.set_seeds(seeds)
    a.seed_latents()
    assert np.array_equal(_bits(a.latents()), _bits(z2))
    b = _open(tsd_mod, diffusion.model, B, sampler, False, steps, z2, ctx, uctx, noise)
    a.step(0), b.step(0)
    assert np.array_equal(_bits(a.latents()), _bits(b.latents()))
    a.close(), b.close()
    # add_noise_seeded(i) == add_noise(i, stream 4); set_inpaint(seeded=True) == set_inpaint(noise = stream 4)
    a = _open(tsd_mod, diffusion.model, B, sampler, False, steps, lat, ctx, uctx, None, start=1)
    a.set_seeds(seeds)
    a.add_noise_seeded(1)
    b = _open(tsd_mod, diffusion.model, B, sampler, False, steps, lat, ctx, uctx, noise[: steps - 1], start=1)
    b.add_noise(1, z4)
    assert np.array_equal(_bits(a.latents()), _bits(b.latents()))
    assert not np.array_equal(a.latents(), lat)
    a.set_inpaint(_mask(B), known, seeded=True)
    b.set_inpaint(_mask(B), known, z4)
    assert a.inpaint_active and b.inpaint_active
    for i in range(2):
        a.step(i), b.step(i)
        assert np.array_equal(_bits(a.latents()), _bits(b.latents())), i
    a.close(), b.close()


# ---- 8. batch invariance ---------------------------------------------------------------------------------------------------------------
def test_a_seed_gives_the_same_sample_wherever_it_sits_in_the_batch(gpu_ctx, tsd_mod, diffusion):
    """Seed s with its context in a B = 1 session, at slot 0 and at slot 2 of a B = 3 session: the same latents after 3 DDPM steps,
    bitwise.  Swapping two seeds (their samples share a context) swaps those samples' results and leaves the third."""
    steps = 4
    s0, s1, s2 = 42, 43, M64
    _, ctx3, _, _ = _inputs(3, tag=1320)
    c0, c1, c2 = ctx3[0], ctx3[1], ctx3[2]

    def run(seeds, ctxs):
        B = len(seeds)
        s = _open(tsd_mod, diffusion.model, B, SAMPLERS[0], False, steps, np.zeros((B, 4, L, L), np.float32), np.stack(ctxs), None, None)
        s.set_seeds(seeds)
        s.seed_latents()
        for i in range(3):
            s.step(i)
        out = s.latents()
        s.close()
        return out

    alone = run([s0], [c0])
    first = run([s0, s1, s2], [c0, c1, c2])
    last = run([s1, s2, s0], [c1, c2, c0])
    assert np.array_equal(_bits(alone[0]), _bits(first[0]))
    assert np.array_equal(_bits(alone[0]), _bits(last[2]))
    assert np.array_equal(_bits(first[1]), _bits(last[0])) and np.array_equal(_bits(first[2]), _bits(last[1]))
    x = run([s0, s1, s2], [c0, c0, c2])
    y = run([s1, s0, s2], [c0, c0, c2])
    assert np.array_equal(_bits(x[0]), _bits(y[1])) and np.array_equal(_bits(x[1]), _bits(y[0])) and np.array_equal(_bits(x[2]), _bits(y[2]))
    assert not np.array_equal(x[0], x[1])


# ---- 9. launch accounting --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("sampler", SAMPLERS[:2], ids=lambda s: s[0])
def test_a_seeded_step_makes_the_launches_of_a_step_with_uploaded_noise(gpu_ctx, tsd_mod, diffusion, sampler, cfg):
    """Per-class launch counts of tsd_ctx_profile_begin / _end over 2 steps that take noise: the inline form shipped, so a seeded step
    makes exactly the launches of an unseeded step with uploaded noise - no fill, no extra elementwise launch."""
    B, steps, P = 2, 4, 2
    lat, ctx, uctx, _ = _inputs(B, tag=1330)
    seeds = [5, 6]

    def profile(seeded):
        s = _open(tsd_mod, diffusion.model, B, sampler, cfg, steps, lat, ctx, uctx, None if seeded else _step_noise(tsd_mod, gpu_ctx, seeds, steps))
        if seeded:
            s.set_seeds(seeds)
        s.step(0)
        gpu_ctx.profile_begin()
        try:
            for i in range(1, 1 + P):
                s.step(i)
        finally:
            prof = gpu_ctx.profile_end()
        s.close()
        return {k: n for k, (_, n) in prof.items()}

    off, on = profile(False), profile(True)
    print(f"[noise] {sampler[0]} cfg={cfg}: launches per step {sum(off.values()) // P} uploaded noise, {sum(on.values()) // P} seeded")
    assert on == off, (on, off)


# ---- 10. the state machine -------------------------------------------------------------------------------------------------------------
def test_state_machine(gpu_ctx, tsd_mod, diffusion):
    from tsd._lib import TSD_E_ARG, TSD_E_STATE, TSD_OK, ptr
    lib = tsd_mod._lib.lib()
    B, steps = 2, 4
    lat, ctx, uctx, known = _inputs(B, tag=1340)
    seeds = (C.c_uint64 * B)(3, 4)
    mask = _mask(B)
    s = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=False)
    s.set_schedule(N_TRAIN, steps, 0)
    # before upload()
    assert lib.tsd_session_set_seeds(s.h, seeds) == TSD_E_STATE and lib.tsd_session_set_seeds(s.h, None) == TSD_E_STATE
    assert lib.tsd_session_seeds_active(s.h) == 0
    assert lib.tsd_session_seed_latents(s.h) == TSD_E_STATE and lib.tsd_session_add_noise_seeded(s.h, 0) == TSD_E_STATE
    assert lib.tsd_session_set_inpaint_seeded(s.h, ptr(mask), ptr(known)) == TSD_E_STATE
    # an upload with a noise tensor: one source of noise per upload
    s.upload(lat, ctx, None, rng.normal(SEED, 1345, steps * B * CHW).reshape(steps, B, 4, L, L))
    assert lib.tsd_session_set_seeds(s.h, seeds) == TSD_E_STATE and not s.seeds_active
    assert lib.tsd_session_set_seeds(s.h, None) == TSD_OK
    # without seeds
    s.upload(lat, ctx, None, None)
    assert lib.tsd_session_seed_latents(s.h) == TSD_E_STATE and lib.tsd_session_add_noise_seeded(s.h, 0) == TSD_E_STATE
    assert lib.tsd_session_set_inpaint_seeded(s.h, ptr(mask), ptr(known)) == TSD_E_STATE and not s.inpaint_active
    assert np.array_equal(_bits(s.latents()), _bits(lat))   # the refused calls changed nothing
    # on, and what turns it off
    s.set_seeds([3, 4])
    assert s.seeds_active
    assert lib.tsd_session_add_noise_seeded(s.h, -1) == TSD_E_ARG and lib.tsd_session_add_noise_seeded(s.h, steps) == TSD_E_ARG
    bad = mask.copy()
    bad[0, 0, 0] = 1.5
    assert lib.tsd_session_set_inpaint_seeded(s.h, ptr(bad), ptr(known)) == TSD_E_ARG and not s.inpaint_active
    assert lib.tsd_session_set_inpaint_seeded(s.h, ptr(mask), None) == TSD_E_ARG
    s.set_inpaint(mask, known, seeded=True)
    assert s.inpaint_active
    s.set_inpaint(None, seeded=True)
    assert not s.inpaint_active and s.seeds_active
    s.set_seeds(None)
    assert not s.seeds_active
    s.set_seeds([3, 4])
    s.upload(lat, ctx, None, None)
    assert not s.seeds_active
    s.set_seeds([3, 4])
    s.set_schedule(N_TRAIN, steps, 0)
    assert not s.seeds_active and lib.tsd_session_set_seeds(s.h, seeds) == TSD_E_STATE
    s.upload(lat, ctx, None, None)
    s.set_seeds([3, 4])
    s.set_sampler("ddim", 0.5, "trailing")
    assert not s.seeds_active
    with pytest.raises(ValueError):
        s.set_seeds([1])
    with pytest.raises(ValueError):
        s.set_seeds([1, 1 << 64])
    s.close()
    # NULL session
    assert lib.tsd_session_set_seeds(None, seeds) == TSD_E_ARG and lib.tsd_session_seeds_active(None) == TSD_E_ARG
    assert lib.tsd_session_seed_latents(None) == TSD_E_ARG and lib.tsd_session_add_noise_seeded(None, 0) == TSD_E_ARG
    assert lib.tsd_session_set_inpaint_seeded(None, ptr(mask), ptr(known)) == TSD_E_ARG
    # DPM-Solver++(2M) with seeds equals without them, second-order steps included
    outs = []
    for seeded in (False, True):
        d = _open(tsd_mod, diffusion.model, B, SAMPLERS[2], False, steps, lat, ctx, None, None)
        if seeded:
            d.set_seeds([3, 4])
        for i in range(steps):
            d.step(i)
        outs.append(d.latents())
        d.close()
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


# ---- 11. generate(seeds=...) -----------------------------------------------------------------------------------------------------------
def test_generate_with_seeds_is_reproducible_per_sample(gpu_ctx, tsd_mod, diffusion):
    B = 2
    _, ctx, uctx, _ = _inputs(B, tag=1350)
    dec = tsd_mod.Decoder(seed=SEED)
    kw = dict(uncond_context=uctx, cfg=True, inference_steps=3, L=L)
    a, b, c = 101, 102, 103
    im1 = tsd_mod.generate(diffusion, dec, ctx, seeds=[a, b], **kw)
    im2 = tsd_mod.generate(diffusion, dec, ctx, seeds=[a, b], **kw)
    im3 = tsd_mod.generate(diffusion, dec, ctx, seeds=[a, c], **kw)
    assert im1.shape == (B, 3, 8 * L, 8 * L) and np.isfinite(im1).all()
    assert np.array_equal(_bits(im1), _bits(im2))
    assert np.array_equal(_bits(im1[0]), _bits(im3[0])) and not np.array_equal(im1[1], im3[1])
    # img2img and inpainting take the seeded entries too (only the encoder's noise stays a host tensor)
    enc = tsd_mod.Encoder(seed=SEED)
    image = (rng.uniform(SEED, 1356, B * 3 * 64 * L * L, 1.0).reshape(B, 3, 8 * L, 8 * L) + 1.0) * 127.5
    mask = np.zeros((B, 8 * L, 8 * L), dtype=np.float32)
    mask[:, :, : 4 * L] = 1.0
    kw2 = dict(kw, input_image=image, encoder=enc, strength=0.7, return_latents=True)
    for extra in ({}, {"mask": mask}):
        l1 = tsd_mod.generate(diffusion, None, ctx, seeds=[a, b], **kw2, **extra)
        l2 = tsd_mod.generate(diffusion, None, ctx, seeds=[a, b], **kw2, **extra)
        l3 = tsd_mod.generate(diffusion, None, ctx, seeds=[a, c], **kw2, **extra)
        assert np.isfinite(l1).all() and np.array_equal(_bits(l1), _bits(l2))
        assert np.array_equal(_bits(l1[0]), _bits(l3[0])) and not np.array_equal(l1[1], l3[1])
