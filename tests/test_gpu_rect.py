"""GPU tests of rectangular latents: every entry point at LH != LW, in both orientations so that a swapped H / W cannot cancel.
Model parity is against the numpy oracle with the model tolerances of tests/util.py; everything a session adds on top of the UNet
(samplers, seeds, inpainting, slots, CFG) is held bitwise to a composition of calls that other tests hold to float64.
Tiny-SD at random init (seed 1234) unless a test says otherwise; T = 77."""
import ctypes as C

import numpy as np
import pytest

from inpaint_ref import MASK_ANY, MASK_AREA, blend_scalars, coeffs, host_step, known_f32
from oracle import models, ops, rng, sampler, spec
from sampler_ref import N_TRAIN
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, rel_l2

pytestmark = pytest.mark.gpu
SEED = 1234
T = 77


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


@pytest.fixture(scope="module")
def decoder(gpu_ctx, tsd_mod):
    return tsd_mod.Decoder(seed=SEED)


@pytest.fixture(scope="module")
def encoder(gpu_ctx, tsd_mod):
    return tsd_mod.Encoder(seed=SEED)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _inputs(B, LH, LW, tag):
    lat = rng.normal(SEED, tag, B * 4 * LH * LW).reshape(B, 4, LH, LW)
    ctx = rng.normal(SEED, tag + 1, B * T * 768).reshape(B, T, 768)
    return lat, ctx


def _tembs(B):
    return np.stack([ops.time_embedding(t) for t in (980.0, 430.0, 20.0)[:B]])


# ---- 1. UNet parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,LH,LW", [(2, 8, 16), (2, 16, 8), (3, 16, 24), (3, 24, 16)])
def test_unet_matches_oracle(B, LH, LW, diffusion, unet_params):
    """(8,16) / (16,8): 128 / 32 / 8 tokens per level.  (16,24) / (24,16): 384 / 96 / 24 tokens - the fused attention head / tail run
    at the first level, the fallbacks at the other two - and there a sample computed alone equals its row of the batch bit for bit."""
    lat, ctx = _inputs(B, LH, LW, tag=2000 + LH)
    temb = _tembs(B)
    out = diffusion.forward(lat, ctx, temb)
    assert out.shape == (B, 4, LH, LW)
    ref = np.stack([models.diffusion(unet_params, lat[b], ctx[b], temb[b]) for b in range(B)])
    assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, f"Diffusion.forward B={B} {LH}x{LW}")
    if B == 3:
        single = np.asarray(diffusion.forward(lat[1], ctx[1], temb[1]))
        assert _same(single.reshape(out[1].shape), out[1])


# ---- 2. one large case ----------------------------------------------------------------------------------------------------------------
def test_unet_at_48x80_matches_oracle_and_its_unfused_graph(gpu_ctx, tsd_mod, diffusion, unet_params):
    """3840 tokens per sample: the smallest size here at which the attention plan picks the eight-wave flash kernel, and the
    loader-wave / staggered conv tiles see a non-square level.  Against the oracle, and the fused attention blocks against the
    op-by-op graph on the same inputs (the bound of test_fused_attention_blocks_match_unfused_graph_at_full_size)."""
    from tsd._lib import lib
    LH, LW = 48, 80
    lat, ctx = _inputs(1, LH, LW, tag=2100)
    temb = ops.time_embedding(430.0)[None]
    old = lib().tsd_debug_set_fused_attention(gpu_ctx.h, 1)
    try:
        fused = diffusion.forward(lat, ctx, temb)
        lib().tsd_debug_set_fused_attention(gpu_ctx.h, 0)
        plain = diffusion.forward(lat, ctx, temb)
    finally:
        lib().tsd_debug_set_fused_attention(gpu_ctx.h, old)
    assert np.isfinite(fused).all() and np.isfinite(plain).all()
    err = rel_l2(fused, plain)
    print(f"[parity] fused vs op-by-op attention blocks, B=1 48x80: rel_l2 = {err:.3e}")
    assert err < 3e-3
    ref = models.diffusion(unet_params, lat[0], ctx[0], temb[0])[None]
    assert_close(fused, ref, TOL_MODEL, TOL_MODEL_MAX, "Diffusion.forward B=1 48x80")


@pytest.mark.parametrize("LH,LW", [(64, 96), (96, 64)])
def test_unet_at_512x768_fused_graph_matches_its_unfused_graph(gpu_ctx, tsd_mod, diffusion, LH, LW):
    """6144 tokens at the first level are 192 statistics slabs of 32 rows: more than the 128 a GEMM epilogue emits for, fewer than the
    256 from which the pre-reduction starts.  The fused attention tail emits them all the same and the next GroupNorm finishes them in
    two trips of its loop; the op-by-op graph runs a statistics pass there instead.  The oracle is too slow at this size: the two graphs
    against each other (the bound of the square test at 64x64), the fused one repeatable and batch invariant bit for bit."""
    from tsd._lib import lib
    lat, ctx = _inputs(2, LH, LW, tag=2150 + LH)
    temb = _tembs(2)
    old = lib().tsd_debug_set_fused_attention(gpu_ctx.h, 1)
    try:
        fused = diffusion.forward(lat, ctx, temb)
        assert _same(diffusion.forward(lat, ctx, temb), fused)
        assert _same(np.asarray(diffusion.forward(lat[1], ctx[1], temb[1])).reshape(fused[1].shape), fused[1])
        lib().tsd_debug_set_fused_attention(gpu_ctx.h, 0)
        plain = diffusion.forward(lat, ctx, temb)
    finally:
        lib().tsd_debug_set_fused_attention(gpu_ctx.h, old)
    assert fused.shape == (2, 4, LH, LW) and np.isfinite(fused).all() and np.isfinite(plain).all()
    err = rel_l2(fused, plain)
    print(f"[parity] fused vs op-by-op attention blocks, B=2 {LH}x{LW}: rel_l2 = {err:.3e}")
    assert err < 3e-3


# ---- 3. full-size UNet ----------------------------------------------------------------------------------------------------------------
def test_full_size_unet_matches_oracle_at_16x32(gpu_ctx, tsd_mod):
    d = tsd_mod.Diffusion(seed=SEED, variant="diffusion_sd15")
    try:
        P = spec.init_params("diffusion_sd15", SEED, only_used=True)
        lat, ctx = _inputs(1, 16, 32, tag=2200)
        temb = ops.time_embedding(430.0)[None]
        out = d.forward(lat, ctx, temb)
        ref = models.diffusion_sd15(P, lat[0], ctx[0], temb[0])[None]
        del P
        assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, "full-size Diffusion.forward 16x32")
        with pytest.raises(tsd_mod.TsdError):      # 24 is a multiple of 8, not of 16
            d.forward(np.zeros((1, 4, 16, 24), np.float32), ctx, temb)
    finally:
        d.model.close()


# ---- 4. VAE ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LH,LW", [(8, 16), (16, 8)])
def test_decoder_matches_oracle(LH, LW, decoder):
    P = spec.init_params("decoder", SEED, only_used=True)
    lat = rng.normal(SEED, 2300 + LH, 2 * 4 * LH * LW).reshape(2, 4, LH, LW) * 0.18215
    out = decoder.forward(lat)
    assert out.shape == (2, 3, 8 * LH, 8 * LW)
    ref = np.stack([models.decoder(P, lat[b]) for b in range(2)])
    assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, f"Decoder.forward {LH}x{LW}")


@pytest.mark.parametrize("SH,SW", [(64, 128), (128, 64)])
def test_encoder_matches_oracle(SH, SW, encoder):
    P = spec.init_params("encoder", SEED, only_used=True)
    img = rng.uniform(SEED, 2400 + SH, 3 * SH * SW, 1.0).reshape(1, 3, SH, SW)
    noise = rng.normal(SEED, 2401 + SH, 4 * (SH // 8) * (SW // 8)).reshape(1, 4, SH // 8, SW // 8)
    out = encoder.forward(img, noise)
    assert out.shape == (1, 4, SH // 8, SW // 8)
    ref = models.encoder(P, img[0], noise[0])[None]
    assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, f"Encoder.forward {SH}x{SW}")


# ---- 5. session against the oracle ----------------------------------------------------------------------------------------------------
def test_session_denoise_matches_oracle(gpu_ctx, tsd_mod, diffusion, unet_params):
    B, LH, LW, steps = 1, 8, 16, 3
    lat, ctx = _inputs(B, LH, LW, tag=2500)
    noise = rng.normal(SEED, 2502, steps * B * 4 * LH * LW).reshape(steps, B, 4, LH, LW)
    s = tsd_mod.Session(diffusion.model, None, B, (LH, LW), T, cfg=False)
    assert (s.L, s.LH, s.LW) == ((LH, LW), LH, LW)
    lh, lw = C.c_int(0), C.c_int(0)
    assert tsd_mod._lib.lib().tsd_session_shape(s.h, C.byref(lh), C.byref(lw)) == 0 and (lh.value, lw.value) == (LH, LW)
    s.set_schedule(N_TRAIN, steps, 0)
    s.upload(lat, ctx, None, noise)
    for i in range(steps):
        s.step(i)
    out = s.latents()
    s.close()
    ref = sampler.denoise(unet_params, lat[0], ctx[0], steps, noise[:, 0])[None]
    assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, "session 3 DDPM steps 8x16")


# ---- 6. CFG ---------------------------------------------------------------------------------------------------------------------------
def test_cfg_batch_equals_two_passes(gpu_ctx, tsd_mod, diffusion):
    """One UNet call on 2B then the combine == two passes of B (the statement and the bound of the square test in test_gpu_models.py)."""
    B, LH, LW = 1, 16, 8
    lat, ctx = _inputs(B, LH, LW, tag=2600)
    _, uctx = _inputs(B, LH, LW, tag=2610)
    s = tsd_mod.Session(diffusion.model, None, B, (LH, LW), T, cfg=True)
    s.set_schedule(N_TRAIN, 2, 0)
    s.upload(lat, ctx, uctx, None, cfg_scale=7.5)
    s.step(0)
    got = s.latents()
    s.close()
    temb = tsd_mod.get_time_embedding(500.0).reshape(1, 320)
    e_c = diffusion.forward(lat, ctx, temb)
    e_u = diffusion.forward(lat, uctx, temb)
    sm = sampler.DDPMSampler(N_TRAIN)
    sm.set_inference_timesteps(2)
    ref = sm.step(500, lat, sampler.cfg_combine(e_c, e_u, 7.5), np.zeros_like(lat))
    assert rel_l2(got, ref) < 1e-5


# ---- 7. samplers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,eta,spacing", [("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")], ids=["ddim", "dpmpp_2m"])
def test_sampler_session_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, diffusion, kind, eta, spacing):
    """The session's step is the UNet forward (bitwise batch invariant: the CFG batch of 2B equals two passes) and tsd_sampler_step_f32's
    kernel on tsd_sampler_coeffs' scalars: the latents after every step ARE those of that loop driven from the host."""
    B, LH, LW, steps = 2, 8, 16, 3
    lat, ctx = _inputs(B, LH, LW, tag=2700)
    _, uctx = _inputs(B, LH, LW, tag=2710)
    noise = rng.normal(SEED, 2720, steps * B * 4 * LH * LW).reshape(steps, B, 4, LH, LW)
    s = tsd_mod.Session(diffusion.model, None, B, (LH, LW), T, cfg=True)
    s.set_sampler(kind, eta, spacing)
    s.set_schedule(N_TRAIN, steps, 0)
    s.upload(lat, ctx, uctx, noise, cfg_scale=7.5)
    x, hist = lat, None
    multistep = kind == "dpmpp_2m"
    for i in range(steps):
        s.step(i)
        got = s.latents()
        cd = coeffs(tsd_mod, kind, eta, spacing, steps, i, hist is not None)
        assert int(cd[0]) == s.timestep(i)
        x, h = host_step(tsd_mod, gpu_ctx, diffusion, x, ctx, uctx, 7.5, int(cd[0]), cd, hist, noise[i], multistep)
        hist = h if multistep else None
        assert _same(got, x), (kind, i, float(np.abs(got - x).max()))
    s.close()


# ---- 8. seeds -------------------------------------------------------------------------------------------------------------------------
def test_seeded_session_is_the_session_that_uploads_the_streams(gpu_ctx, tsd_mod, diffusion):
    """The counter of the seeded noise is the element's index inside its sample, (c LH + y) LW + x: stream 16 + i of seeds[b], read as
    (4, LH, LW), is the noise tensor of step i.  And a seed's sample does not depend on its batch position or on B."""
    B, LH, LW, steps = 2, 8, 16, 3
    chw = 4 * LH * LW
    lat, ctx = _inputs(B, LH, LW, tag=2800)
    seeds = [1000003, 77]

    def run(order, seeded):
        nb = len(order)
        s = tsd_mod.Session(diffusion.model, None, nb, (LH, LW), T, cfg=False)
        s.set_schedule(N_TRAIN, steps, 0)
        noise = None
        if not seeded:
            noise = np.stack([np.stack([tsd_mod.normal_fill(seeds[b], 16 + i, chw, ctx=gpu_ctx).reshape(4, LH, LW) for b in order])
                              for i in range(steps)])
        s.upload(lat[order], ctx[order], None, noise)
        if seeded:
            s.set_seeds([seeds[b] for b in order])
        for i in range(steps):
            s.step(i)
        out = s.latents()
        s.close()
        return out

    a = run([0, 1], True)
    assert np.isfinite(a).all() and _same(a, run([0, 1], False))
    swapped = run([1, 0], True)
    assert _same(swapped[0], a[1]) and _same(swapped[1], a[0])
    assert _same(run([1], True)[0], a[1])
    assert not _same(a[0], a[1])


# ---- 9. the mask kernel ---------------------------------------------------------------------------------------------------------------
def test_latent_mask_is_exact(gpu_ctx, tsd_mod):
    """Random pixel values on the grid k / 256: every partial sum of 64 of them is a multiple of 2^-8 below 2^6, exact in fp32 in any
    order, so the kernel's block mean must EQUAL the float64 mean; `any` is the threshold of the block maximum at 0.5."""
    from tsd._lib import f32, ptr
    B, LH, LW = 2, 8, 16
    px = np.floor(rng.uniform(SEED, 2900, B * 64 * LH * LW, 1.0).reshape(B, 8 * LH, 8 * LW) * 128.0 + 128.0) / 256.0
    px = np.clip(px, 0.0, 1.0).astype(np.float32)
    px[0, :8, 8:16] = 0.25          # a block with no pixel at or above 0.5: `any` must say 0 for cell (0, 1) of sample 0 only
    blocks = px.astype(np.float64).reshape(B, LH, 8, LW, 8).transpose(0, 1, 3, 2, 4).reshape(B, LH, LW, 64)
    want = {MASK_AREA: blocks.mean(axis=-1), MASK_ANY: (blocks.max(axis=-1) >= 0.5).astype(np.float64)}
    assert want[MASK_ANY][0, 0, 1] == 0.0 and want[MASK_ANY].sum() == B * LH * LW - 1
    for mode, name in ((MASK_AREA, "area"), (MASK_ANY, "any")):
        out = np.full((B, LH, LW), -1.0, dtype=np.float32)
        assert tsd_mod._lib.lib().tsd_latent_mask_hw_f32(gpu_ctx.h, ptr(f32(px)), B, LH, LW, mode, ptr(out)) == 0
        assert np.array_equal(out.astype(np.float64), want[mode]), name
        assert np.array_equal(tsd_mod.latent_mask(px, name, gpu_ctx), out)
        assert np.array_equal(tsd_mod.latent_mask(px[:, None], name, gpu_ctx), out)
    # the square entry is the LH == LW case of the same kernel
    sq = px[:, :, : 8 * LH]
    sq = np.ascontiguousarray(sq)
    a = np.empty((B, LH, LH), dtype=np.float32)
    b = np.empty((B, LH, LH), dtype=np.float32)
    assert tsd_mod._lib.lib().tsd_latent_mask_f32(gpu_ctx.h, ptr(sq), B, LH, MASK_AREA, ptr(a)) == 0
    assert tsd_mod._lib.lib().tsd_latent_mask_hw_f32(gpu_ctx.h, ptr(sq), B, LH, LH, MASK_AREA, ptr(b)) == 0
    assert _same(a, b)


# ---- 10. inpainting -------------------------------------------------------------------------------------------------------------------
def test_inpainting_holds_the_known_region_and_leaves_the_rest_to_the_sampler(gpu_ctx, tsd_mod, diffusion):
    """A 0 / 1 mask with distinct rows that is not symmetric in any sense (16 x 8).  After every step the cells under m = 0 are
    fl(fl(a_prev known) + fl(s_prev noise)) bit for bit, and the cells under m = 1 are those of a session without inpainting that
    takes the same step from the same latents."""
    B, LH, LW, steps = 2, 16, 8, 3
    n = B * 4 * LH * LW
    lat, ctx = _inputs(B, LH, LW, tag=3000)
    known, z = (rng.normal(SEED, 3003 + k, n).reshape(B, 4, LH, LW).astype(np.float32) for k in range(2))
    noise = rng.normal(SEED, 3006, steps * n).reshape(steps, B, 4, LH, LW)
    cell = np.arange(LH * LW).reshape(LH, LW)
    mask = np.stack([((cell * 3 + b) % 13 < 6).astype(np.float32) for b in range(B)])
    assert len({r.tobytes() for r in mask[0]}) > LW and (mask == 0).any() and (mask == 1).any()   # more distinct rows than columns
    m4 = np.broadcast_to(mask[:, None], (B, 4, LH, LW))
    sampler_cfg = ("ddpm", 0.0, "leading")

    def open_session(latents):
        s = tsd_mod.Session(diffusion.model, None, B, (LH, LW), T, cfg=False)
        s.set_schedule(N_TRAIN, steps, 0)
        s.upload(latents, ctx, None, noise)
        return s

    s = open_session(lat)
    s.set_inpaint(mask, known, z)
    assert s.inpaint_active
    before = lat.astype(np.float32)
    for i in range(steps):
        s.step(i)
        got = s.latents()
        a_prev, s_prev = blend_scalars(tsd_mod, *sampler_cfg, steps, i)
        k = known_f32(known, z, a_prev, s_prev)
        assert np.array_equal(_bits(got)[m4 == 0], _bits(k)[m4 == 0]), i
        plain = open_session(before)
        plain.step(i)
        free = plain.latents()
        plain.close()
        assert np.array_equal(_bits(got)[m4 == 1], _bits(free)[m4 == 1]), i
        assert not np.array_equal(got[m4 == 0], free[m4 == 0])
        before = got
    s.close()
    with pytest.raises(ValueError):
        s2 = open_session(lat)
        try:
            s2.set_inpaint(np.ascontiguousarray(mask.transpose(0, 2, 1)), known, z)
        finally:
            s2.close()


# ---- 11. slots ------------------------------------------------------------------------------------------------------------------------
def test_staggered_slots_equal_lockstep_bitwise(gpu_ctx, tsd_mod, diffusion):
    """B = 3 at 8 x 16 with CFG, 4 DDPM steps.  Slot 0: inpainting img2img from index 0.  Slot 1: img2img from index 1 with guidance
    rescale 0.7.  Slot 2: img2img from index 2.  They start on successive ticks and finish together; each slot's latents are those
    of the same sample of a lockstep session of the same shape running its request."""
    B, LH, LW, steps = 3, 8, 16, 4
    chw = 4 * LH * LW
    scales = (7.5, 3.0, 1.5)
    reqs = [dict(ctx=rng.normal(SEED, 3100 + 10 * k, T * 768).reshape(T, 768), uctx=rng.normal(SEED, 3101 + 10 * k, T * 768).reshape(T, 768),
                 seed=3000017 * (k + 1) + 5, scale=scales[k],
                 lat=rng.normal(SEED, 3102 + 10 * k, chw).reshape(4, LH, LW).astype(np.float32)) for k in range(B)]
    cell = np.arange(LH * LW).reshape(LH, LW)
    v = (cell * 3) % 13
    mask = np.where(v < 4, 0.0, np.where(v > 9, 1.0, v / 16.0)).astype(np.float32)
    assert (mask == 0).any() and (mask == 1).any() and len({r.tobytes() for r in mask}) == LH
    fill_lat = rng.normal(SEED, 3190, B * chw).reshape(B, 4, LH, LW).astype(np.float32)
    fill_ctx, fill_uctx = (rng.normal(SEED, 3191 + k, B * T * 768).reshape(B, T, 768) for k in range(2))
    plan = [(0, 0, True, 0.0), (1, 1, False, 0.7), (2, 2, False, 0.0)]   # (slot = request, start index, inpainting, guidance rescale)

    def lockstep(k, start, inpaint, phi):
        lat, ctx, uctx = fill_lat.copy(), fill_ctx.copy(), fill_uctx.copy()
        lat[k], ctx[k], uctx[k] = reqs[k]["lat"], reqs[k]["ctx"], reqs[k]["uctx"]
        seeds = [91, 92, 93]
        seeds[k] = reqs[k]["seed"]
        s = tsd_mod.Session(diffusion.model, None, B, (LH, LW), T, cfg=True)
        s.set_schedule(N_TRAIN, steps, 0)
        s.upload(lat, ctx, uctx, None, cfg_scale=reqs[k]["scale"])
        s.set_seeds(seeds)
        s.add_noise_seeded(start)
        if inpaint:
            masks = np.ones((B, LH, LW), dtype=np.float32)
            masks[k] = mask
            s.set_inpaint(masks, lat, seeded=True)
        if phi > 0:
            s.set_guidance_rescale(phi)
        for i in range(start, steps):
            s.step(i)
        out = s.latents()[k].copy()
        s.close()
        return out

    s = tsd_mod.Session(diffusion.model, None, B, (LH, LW), T, cfg=True)
    s.set_schedule(N_TRAIN, steps, 0)
    s.slots_open()
    for tick in range(steps):
        if tick < B:
            k, start, inpaint, phi = plan[tick]
            r = reqs[k]
            s.slot_start(k, r["ctx"], r["uctx"], latents=r["lat"], noise_at_start=True, seed=r["seed"], start_index=start, cfg_scale=r["scale"])
            if inpaint:
                s.slot_set_inpaint(k, mask, r["lat"])
            if phi > 0:
                s.slot_set_guidance_rescale(k, phi)
        done = s.advance()
        assert done == ([0, 1, 2] if tick == steps - 1 else []), (tick, done)
    got = [s.slot_latents(k) for k in range(B)]
    s.close()
    for k, start, inpaint, phi in plan:
        assert got[k].shape == (4, LH, LW) and np.isfinite(got[k]).all()
        ref = lockstep(k, start, inpaint, phi)
        assert _same(got[k], ref), (k, float(np.abs(got[k] - ref).max()))
    assert not _same(got[0], lockstep(0, 0, False, 0.0))       # the mask matters
    assert not _same(got[1], lockstep(1, 1, False, 0.0))       # and so does the rescale


# ---- 12. the square case of the new entries is the old entries ------------------------------------------------------------------------
def test_square_calls_through_the_new_entries_give_the_old_entries_bits(gpu_ctx, tsd_mod, diffusion):
    from tsd._lib import check, f32, ptr, vp
    lib = tsd_mod._lib.lib()
    B, L, steps = 2, 16, 2
    lat, ctx = _inputs(B, L, L, tag=3200)
    lat, ctx, temb = f32(lat), f32(ctx), f32(_tembs(B))
    old, new = np.empty_like(lat), np.empty_like(lat)
    check(lib.tsd_diffusion_forward(diffusion.model.h, ptr(lat), ptr(ctx), ptr(temb), B, L, T, ptr(old)))
    check(lib.tsd_diffusion_forward_hw(diffusion.model.h, ptr(lat), ptr(ctx), ptr(temb), B, L, L, T, ptr(new)))
    assert np.isfinite(old).all() and _same(old, new)
    noise = f32(rng.normal(SEED, 3202, steps * B * 4 * L * L).reshape(steps, B, 4, L, L))
    outs = []
    for create_hw in (False, True):
        h = vp()
        if create_hw:
            check(lib.tsd_session_create_hw(diffusion.model.h, None, B, L, L, T, 1, C.byref(h)))
        else:
            check(lib.tsd_session_create(diffusion.model.h, None, B, L, T, 1, C.byref(h)))
        try:
            lh, lw = C.c_int(0), C.c_int(0)
            check(lib.tsd_session_shape(h, C.byref(lh), C.byref(lw)))
            assert (lh.value, lw.value) == (L, L)
            check(lib.tsd_session_set_schedule(h, N_TRAIN, steps, 0))
            check(lib.tsd_session_upload(h, ptr(lat), ptr(ctx), ptr(ctx[::-1].copy()), ptr(noise), 7.5))
            for i in range(steps):
                check(lib.tsd_session_step(h, i))
            out = np.empty_like(lat)
            check(lib.tsd_session_download_latents(h, ptr(out)))
            outs.append(out)
        finally:
            lib.tsd_session_destroy(h)
    assert _same(outs[0], outs[1])


# ---- 13. refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_sides_are_refused_and_nothing_is_touched(gpu_ctx, tsd_mod, diffusion, decoder, encoder):
    from tsd._lib import TSD_E_SHAPE, f32, ptr, vp
    lib = tsd_mod._lib.lib()
    big = f32(np.zeros(4 * 3 * 128 * 128))
    ctx = f32(np.zeros((1, T, 768)))
    temb = f32(np.zeros((1, 320)))
    for lh, lw in ((12, 16), (16, 12), (16, 0), (0, 16), (-8, 16)):
        out = np.full(4 * 3 * 128 * 128, 7.0, dtype=np.float32)
        assert lib.tsd_diffusion_forward_hw(diffusion.model.h, ptr(big), ptr(ctx), ptr(temb), 1, lh, lw, T, ptr(out)) == TSD_E_SHAPE, (lh, lw)
        assert lib.tsd_decoder_forward_hw(decoder.model.h, ptr(big), 1, lh, lw, ptr(out)) == TSD_E_SHAPE, (lh, lw)
        h = vp()
        assert lib.tsd_session_create_hw(diffusion.model.h, None, 1, lh, lw, T, 0, C.byref(h)) == TSD_E_SHAPE and not h.value, (lh, lw)
        assert (out == 7.0).all()
    for sh, sw in ((96, 128), (128, 96), (64, 0)):
        out = np.full(4 * 16 * 16, 7.0, dtype=np.float32)
        assert lib.tsd_encoder_forward_hw(encoder.model.h, ptr(big), ptr(big), 1, sh, sw, ptr(out)) == TSD_E_SHAPE, (sh, sw)
        assert (out == 7.0).all()
    out = np.full(16, 7.0, dtype=np.float32)
    assert lib.tsd_latent_mask_hw_f32(gpu_ctx.h, ptr(big), 1, 2, 0, 0, ptr(out)) == TSD_E_SHAPE and (out == 7.0).all()
    # Python: an array of the transposed shape is refused before the library reads it
    LH, LW = 8, 16
    lat, cx = _inputs(1, LH, LW, tag=3300)
    s = tsd_mod.Session(diffusion.model, None, 1, (LH, LW), T, cfg=False)
    try:
        s.set_schedule(N_TRAIN, 2, 0)
        with pytest.raises(ValueError):
            s.upload(np.ascontiguousarray(lat.transpose(0, 1, 3, 2)), cx, None, None)
        with pytest.raises(ValueError):
            s.upload(lat, cx, None, np.zeros((2, 1, 4, LW, LH), np.float32))
        s.upload(lat, cx, None, None)
        with pytest.raises(ValueError):
            s.add_noise(0, np.zeros((1, 4, LW, LH), np.float32))
    finally:
        s.close()
    with pytest.raises(ValueError):
        tsd_mod.Session(diffusion.model, None, 1, (8, 16, 24), T)
    with pytest.raises(ValueError):
        tsd_mod.generate(diffusion, None, cx, cfg=False, inference_steps=2, L=(8, -16))


# ---- 14. end to end -------------------------------------------------------------------------------------------------------------------
def test_generate_equals_its_manual_composition(gpu_ctx, tsd_mod, diffusion, decoder, encoder):
    from tsd.utils import _unary
    B, LH, LW, steps, seed_val = 2, 8, 16, 3, 11
    nl = B * 4 * LH * LW
    _, ctx = _inputs(B, LH, LW, tag=3400)
    img = tsd_mod.generate(diffusion, decoder, ctx, cfg=False, inference_steps=steps, seed_val=seed_val, L=(LH, LW))
    assert img.shape == (B, 3, 8 * LH, 8 * LW) and np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 255.0
    # by hand: generate's default latents and noise, a session's steps, Decoder.forward, the rescale
    s = tsd_mod.Session(diffusion.model, None, B, (LH, LW), T, cfg=False)
    s.set_schedule(N_TRAIN, steps, 0)
    s.upload(tsd_mod.rng.normal(seed_val, 2, nl).reshape(B, 4, LH, LW), ctx, None,
             tsd_mod.rng.normal(seed_val, 3, steps * nl).reshape(steps, B, 4, LH, LW))
    for i in range(steps):
        s.step(i)
    lat = s.latents()
    s.close()
    by_hand = _unary("tsd_rescale_images_f32", decoder.forward(lat), gpu_ctx)
    assert _same(img, np.asarray(by_hand).reshape(img.shape))
    # img2img with a pixel mask: the kept latent cells end on the encoder's latents bit for bit (the last blend is 1 * known + 0 * noise)
    src = rng.uniform(SEED, 3410, B * 3 * 64 * LH * LW, 1.0).reshape(B, 3, 8 * LH, 8 * LW) * 127.5 + 127.5
    mask = np.zeros((B, 8 * LH, 8 * LW), dtype=np.float32)
    mask[:, :, : 8 * LW // 2 + 3] = 1.0      # the left half and 3 pixels of the next cell column: `any` regenerates that column too
    kw = dict(cfg=False, inference_steps=steps, seed_val=seed_val, L=(LH, LW), input_image=src, encoder=encoder, mask=mask, strength=1.0)
    out = tsd_mod.generate(diffusion, decoder, ctx, **kw)
    assert out.shape == (B, 3, 8 * LH, 8 * LW) and np.isfinite(out).all()
    lat_out = tsd_mod.generate(diffusion, decoder, ctx, return_latents=True, **kw)
    known = encoder.forward(tsd_mod.rescale(src, (0, 255), (-1, 1)), tsd_mod.rng.normal(seed_val, 1, nl).reshape(B, 4, LH, LW))
    keep = LW // 2 + 1
    assert _same(lat_out[:, :, :, keep:], known[:, :, :, keep:])
    assert not np.array_equal(lat_out[:, :, :, :keep], known[:, :, :, :keep])
    with pytest.raises(ValueError):
        tsd_mod.generate(diffusion, decoder, ctx, **dict(kw, mask=np.ascontiguousarray(mask.transpose(0, 2, 1))))
