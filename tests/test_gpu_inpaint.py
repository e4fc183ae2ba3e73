"""GPU tests of masked denoising (inpainting): the blend kernel against fp64 with a forward error bound and its exact ends, the
latent-mask kernel against numpy, the session against the unmasked session (all-ones mask), against the known region (all-zeros mask),
against a host-driven loop over the same kernels (bitwise) and against the oracle UNet driven in fp64, the state machine,
`generate(mask=...)` and the launch accounting."""
import numpy as np
import pytest

from inpaint_ref import (MASK_ANY, MASK_AREA, U, blend_f64, blend_op, blend_raw, blend_scalars, coeffs, host_step, known_f32, latent_mask_np,
                         latent_mask_raw, mask_per_element)
from oracle import models, ops, rng
from sampler_ref import N_TRAIN, Papers
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, randn, uni

pytestmark = pytest.mark.gpu
SEED = 1234
SAMPLERS = [("ddpm", 0.0, "leading"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")]
BLEND_ROUNDINGS = 5  # stated above k_inpaint_blend (kernels_sampler.hip)


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


@pytest.fixture(scope="module")
def decoder(gpu_ctx, tsd_mod):
    return tsd_mod.Decoder(seed=SEED)


@pytest.fixture(scope="module")
def encoder(gpu_ctx, tsd_mod):
    return tsd_mod.Encoder(seed=SEED)


def _inputs(B, L, T=77, tag=1100):
    """latents, context, uncond context, known latents, their noise"""
    n = B * 4 * L * L
    lat, known, z = (rng.normal(SEED, tag + k, n).reshape(B, 4, L, L) for k in (0, 3, 4))
    ctx, uctx = (rng.normal(SEED, tag + k, B * T * 768).reshape(B, T, 768) for k in (1, 2))
    return lat, ctx, uctx, known, z


def _mixed_mask(B, L):
    """binary blocks plus a soft border: the left half is regenerated, the right half kept, the two columns between them are soft, and
    sample b's top row is flipped so that the samples differ"""
    m = np.zeros((B, L, L), dtype=np.float32)
    m[:, :, : L // 2 - 1] = 1.0
    m[:, :, L // 2 - 1] = 0.75
    m[:, :, L // 2] = 0.3
    for b in range(B):
        m[b, b % L] = 1.0 - m[b, b % L]
    return m


def _open(tsd_mod, model, B, L, sampler, cfg, steps, lat, ctx, uctx, noise=None, start=0):
    s = tsd_mod.Session(model, None, B, L, 77, cfg=cfg)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, steps, start)
    s.upload(lat, ctx, uctx if cfg else None, noise, cfg_scale=7.5)
    return s


def _step_noise(B, L, steps, tag):
    return rng.normal(SEED, tag, steps * B * 4 * L * L).reshape(steps, B, 4, L, L)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the blend kernel against fp64, element-wise ----------------------------------------------------------------------------------
def test_blend_matches_fp64_within_the_forward_error_bound_and_has_exact_ends(gpu_ctx, tsd_mod):
    """x' = m x + (1 - m)(a known + s noise) at B = 3, hw = 5839 (a prime: n = 70068 is no multiple of the 256-thread block, batch and
    channel boundaries fall inside blocks), with a third of the mask exactly 0, a third exactly 1 and a third in (0, 1), the float
    scalars of a real schedule step and the pair (1, 0), with and without noise, in place and not.

    Bound (forward error of a fixed sequence of fp32 operations, each one rounding, 2^-24 relative): k 2^-24 (|m x| + |1 - m| (|a known| +
    |s noise|)), k the roundings that reach the output through its worst term, counted from k_inpaint_blend's source (fma contraction
    is off there):
      a * known (1) -> + s * noise (2) -> * (1 - m), which carries the rounding of the difference itself (3, 4) -> + m x (5)      k = 5
    (s * noise takes the same path; m x sees 2).  The fp64 side takes the float scalars and the float mask as the kernel does, so the
    bound has no term for them.

    Exact ends: where m == 1 the output is x bitwise, where m == 0 it is fl(fl(a known) + fl(s noise)) bitwise."""
    B, hw = 3, 5839
    x, known, z = (randn(1110 + k, B, 4, hw).astype(np.float32) for k in range(3))
    soft = (uni(1113, 0.5, B * hw) + 0.5).astype(np.float32)
    cls = (np.arange(B * hw) * 7 + 3) % 3
    mask = np.where(cls == 0, np.float32(0), np.where(cls == 1, np.float32(1), soft)).astype(np.float32).reshape(B, hw)
    M = mask_per_element(mask, x.shape)
    ones, zeros = M == 1.0, M == 0.0
    assert ones.sum() > 20000 and zeros.sum() > 20000 and (~ones & ~zeros).sum() > 20000
    worst = 0.0
    for a_prev, s_prev in (blend_scalars(tsd_mod, "ddim", 0.0, "leading", 20, 5), (np.float32(1.0), np.float32(0.0))):
        for noise in (z, None):
            ref, terms = blend_f64(x, mask, known, noise, a_prev, s_prev)
            k32 = known_f32(known, noise, a_prev, s_prev)
            for alias in (False, True):
                rc, got = blend_raw(tsd_mod, gpu_ctx, x, mask, known, noise, a_prev, s_prev, alias=alias)
                assert rc == 0, tsd_mod._lib.last_error()
                err, bound = np.abs(got.astype(np.float64) - ref), BLEND_ROUNDINGS * U * terms
                ratio = float((err[bound > 0] / bound[bound > 0]).max())
                worst = max(worst, ratio)
                print(f"[inpaint] blend a={float(a_prev):.6f} s={float(s_prev):.6f} noise={noise is not None} in place={alias}: "
                      f"worst error / bound {ratio:.3f}")
                assert (err <= bound).all(), (float(a_prev), noise is not None, alias, ratio)
                assert np.array_equal(_bits(got)[ones], _bits(x)[ones])
                assert np.array_equal(_bits(got)[zeros], _bits(k32)[zeros])
    print(f"[inpaint] blend: worst error / bound {worst:.3f} (k = {BLEND_ROUNDINGS})")


# ---- 2. the blend counts non-finite output ----------------------------------------------------------------------------------------------
def test_blend_counts_non_finite_outputs(gpu_ctx, tsd_mod):
    """An inf in x under m == 0 is 0 * inf = NaN in the output: counted and reported (and the count cleared), never replaced."""
    from tsd._lib import TSD_E_NONFINITE, TSD_OK
    lib = tsd_mod._lib.lib()
    B, hw = 1, 250
    x, known, z = (randn(1120 + k, B, 4, hw).astype(np.float32) for k in range(3))
    mask = np.zeros((B, hw), dtype=np.float32)
    mask[0, ::2] = 1.0
    assert lib.tsd_debug_nonfinite_count(gpu_ctx.h, 1) >= 0
    bad = x.copy()
    bad[0, 2, 7] = np.inf            # mask[0, 7] == 0
    rc, got = blend_raw(tsd_mod, gpu_ctx, bad, mask, known, z, 0.8, 0.6)
    assert rc == TSD_E_NONFINITE
    assert lib.tsd_debug_nonfinite_count(gpu_ctx.h, 0) == 0
    rc, got = blend_raw(tsd_mod, gpu_ctx, x, mask, known, z, 0.8, 0.6)
    assert rc == TSD_OK and np.isfinite(got).all()


# ---- 3. the latent mask -----------------------------------------------------------------------------------------------------------------
def test_latent_mask(gpu_ctx, tsd_mod):
    """B = 2, L = 8.  Binary masks: both modes are numpy's bits (a sum of at most 64 ones is exact in any order, times 2^-6 is exact).
    Soft masks: AREA within 64 2^-24 relative of the fp64 mean - 63 additions of non-negative values, each one rounding, so
    sum |v| = sum v and the scaling by 2^-6 is exact.  ANY: a single pixel of 0.5 in a block gives 1, of 0.49 gives 0."""
    from tsd._lib import TSD_E_ARG, TSD_E_SHAPE
    B, L = 2, 8
    S = 8 * L
    binary = (uni(1130, 1.0, B, S, S) > 0.9).astype(np.float32)   # sparse enough that some blocks are empty
    for mode in (MASK_AREA, MASK_ANY):
        rc, got = latent_mask_raw(tsd_mod, gpu_ctx, binary, B, L, mode)
        assert rc == 0, tsd_mod._lib.last_error()
        ref = latent_mask_np(binary, mode).astype(np.float32)
        assert np.array_equal(_bits(got), _bits(ref)), mode
        assert 0 < (ref == 0).sum() < ref.size
    assert np.array_equal(tsd_mod.latent_mask(binary[:, None], "any"), latent_mask_np(binary, MASK_ANY))
    assert np.array_equal(tsd_mod.latent_mask(binary, "area"), latent_mask_np(binary, MASK_AREA).astype(np.float32))

    soft = (uni(1131, 0.5, B, S, S) + 0.5).astype(np.float32)
    rc, got = latent_mask_raw(tsd_mod, gpu_ctx, soft, B, L, MASK_AREA)
    assert rc == 0, tsd_mod._lib.last_error()
    ref = latent_mask_np(soft, MASK_AREA)
    ratio = float((np.abs(got.astype(np.float64) - ref) / (64 * U * ref)).max())
    print(f"[inpaint] latent mask, area, soft: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0

    for v, want in ((0.5, 1.0), (0.49, 0.0)):
        one = np.zeros((B, S, S), dtype=np.float32)
        one[1, 8 * 3 + 5, 8 * 6 + 2] = v      # block (3, 6) of sample 1
        rc, got = latent_mask_raw(tsd_mod, gpu_ctx, one, B, L, MASK_ANY)
        assert rc == 0
        expect = np.zeros((B, L, L), dtype=np.float32)
        expect[1, 3, 6] = want
        assert np.array_equal(got, expect), v

    for bad in (1.5, np.nan):
        m = binary.copy()
        m[1, 40, 17] = bad
        assert latent_mask_raw(tsd_mod, gpu_ctx, m, B, L, MASK_ANY)[0] == TSD_E_ARG, bad
    assert latent_mask_raw(tsd_mod, gpu_ctx, binary, B, L, 2)[0] == TSD_E_ARG
    for badL in (0, -8):
        assert latent_mask_raw(tsd_mod, gpu_ctx, binary, B, badL, MASK_ANY)[0] in (TSD_E_SHAPE, TSD_E_ARG)
    rc, got = latent_mask_raw(tsd_mod, gpu_ctx, binary, B, L, MASK_ANY)   # a refused call leaves the context usable
    assert rc == 0 and np.array_equal(got, latent_mask_np(binary, MASK_ANY))


# ---- 4. an all-ones mask is the unmasked session ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=lambda s: s[0])
def test_all_ones_mask_is_the_unmasked_session_bitwise(gpu_ctx, tsd_mod, diffusion, sampler, cfg):
    """m == 1 returns x bitwise, so the blend launch changes nothing: after every step the latents are the unmasked session's."""
    B, L, steps = 2, 8, 4
    lat, ctx, uctx, known, z = _inputs(B, L, tag=1140)
    noise = _step_noise(B, L, steps, 1146)
    got = []
    for masked in (False, True):
        s = _open(tsd_mod, diffusion.model, B, L, sampler, cfg, steps, lat, ctx, uctx, noise)
        if masked:
            s.set_inpaint(np.ones((B, L, L), dtype=np.float32), known, z)
        assert s.inpaint_active == masked
        per_step = []
        for i in range(steps):
            s.step(i)
            per_step.append(s.latents())
        s.close()
        got.append(np.stack(per_step))
    assert np.array_equal(_bits(got[0]), _bits(got[1]))
    assert not np.array_equal(got[0][-1], got[0][-2])


# ---- 5. an all-zeros mask is the known region ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", SAMPLERS, ids=lambda s: s[0])
def test_all_zeros_mask_is_the_renoised_known_latents(gpu_ctx, tsd_mod, diffusion, sampler):
    """m == 0 returns k = fl(fl(a_prev known) + fl(s_prev noise)) bitwise, with the scalars of the timestep the update lands on
    (tsd_sampler_coeffs of step i + 1, rounded to float); after the last step they are (1, 0) and the latents are `known`."""
    B, L, steps = 2, 8, 4
    lat, ctx, uctx, known, z = _inputs(B, L, tag=1150)
    s = _open(tsd_mod, diffusion.model, B, L, sampler, False, steps, lat, ctx, uctx, _step_noise(B, L, steps, 1156))
    s.set_inpaint(np.zeros((B, L, L), dtype=np.float32), known, z)
    for i in range(steps):
        s.step(i)
        a_prev, s_prev = blend_scalars(tsd_mod, *sampler, steps, i)
        assert np.array_equal(_bits(s.latents()), _bits(known_f32(known, z, a_prev, s_prev))), (sampler, i)
    assert (float(a_prev), float(s_prev)) == (1.0, 0.0)
    assert np.array_equal(_bits(s.latents()), _bits(known))
    s.close()


# ---- 6. session == host-driven loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("sampler", [("ddim", 0.0, "leading"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")],
                         ids=["ddim0-leading", "ddim0.5-trailing", "dpmpp_2m-trailing"])
def test_session_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, diffusion, sampler, cfg):
    """UNet forward, tsd_sampler_step_f32 with the host keeping the history, then tsd_inpaint_blend_f32: the same kernels on the same
    scalars as the session's step, so the latents after every step ARE the host loop's.  The history written by step i serves step
    i + 1 (DPM-Solver++ runs second order from step 1 on: the host loop passes its history)."""
    B, L, steps = 2, 8, 4
    kind, eta, spacing = sampler
    lat, ctx, uctx, known, z = _inputs(B, L, tag=1160)
    noise = _step_noise(B, L, steps, 1166)
    mask = _mixed_mask(B, L)
    s = _open(tsd_mod, diffusion.model, B, L, sampler, cfg, steps, lat, ctx, uctx, noise)
    s.set_inpaint(mask, known, z)
    x, hist = lat, None
    multistep = kind == "dpmpp_2m"
    for i in range(steps):
        s.step(i)
        got = s.latents()
        cd = coeffs(tsd_mod, kind, eta, spacing, steps, i, hist is not None)
        assert int(cd[0]) == s.timestep(i)
        if multistep and 0 < i < steps - 1:
            assert cd[6] != 0.0          # second order: the comparison can tell a dropped history
        x, h = host_step(tsd_mod, gpu_ctx, diffusion, x, ctx, uctx if cfg else None, 7.5, int(cd[0]), cd, hist, noise[i], multistep)
        hist = h if multistep else None
        x = blend_op(tsd_mod, gpu_ctx, x, mask, known, z, *blend_scalars(tsd_mod, kind, eta, spacing, steps, i))
        assert np.array_equal(_bits(got), _bits(x)), (sampler, cfg, i, float(np.abs(got - x).max()))
    s.close()


@pytest.mark.parametrize("cfg", [False, True])
def test_ddpm_session_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, diffusion, cfg):
    """DDPM has no op-level step: a second, unmasked session is uploaded with the current latents, steps once, and its output is
    blended on the host through the op."""
    B, L, steps = 2, 8, 4
    sampler = ("ddpm", 0.0, "leading")
    lat, ctx, uctx, known, z = _inputs(B, L, tag=1170)
    noise = _step_noise(B, L, steps, 1176)
    mask = _mixed_mask(B, L)
    s = _open(tsd_mod, diffusion.model, B, L, sampler, cfg, steps, lat, ctx, uctx, noise)
    s.set_inpaint(mask, known, z)
    plain = _open(tsd_mod, diffusion.model, B, L, sampler, cfg, steps, lat, ctx, uctx, noise)
    x = lat
    for i in range(steps):
        s.step(i)
        got = s.latents()
        plain.upload(x, ctx, uctx if cfg else None, noise, cfg_scale=7.5)
        plain.step(i)
        assert not plain.inpaint_active
        x = blend_op(tsd_mod, gpu_ctx, plain.latents(), mask, known, z, *blend_scalars(tsd_mod, *sampler, steps, i))
        assert np.array_equal(_bits(got), _bits(x)), (cfg, i, float(np.abs(got - x).max()))
    s.close()
    plain.close()


# ---- 7. against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
def test_masked_session_matches_the_oracle_loop(gpu_ctx, tsd_mod, diffusion, unet_params, kind):
    """3 steps (666, 333, 0) of the masked device loop vs the oracle UNet driven by the fp64 restatement of the paper's update
    (sampler_ref.Papers) with the blend in fp64, a binary half-image mask, at the project's full-model tolerance."""
    B, L, steps = 1, 8, 3
    lat, ctx, _, known, z = _inputs(B, L, tag=1180)
    mask = np.zeros((B, L, L), dtype=np.float32)
    mask[:, :, : L // 2] = 1.0
    s = _open(tsd_mod, diffusion.model, B, L, (kind, 0.0, "leading"), False, steps, lat, ctx, None)
    ts = [s.timestep(i) for i in range(s.num_steps)]
    assert ts == [666, 333, 0]
    s.set_inpaint(mask, known, z)
    for i in range(steps):
        s.step(i)
    out = s.latents()
    s.close()
    P = Papers(ts)
    update = P.ddim(0.0) if kind == "ddim" else P.dpmpp_2m
    M = mask[0][None].astype(np.float64)
    x, x0_prev = lat[0].astype(np.float64), None
    for i, t in enumerate(ts):
        eps = models.diffusion(unet_params, x.astype(np.float32), ctx[0], ops.time_embedding(float(t))).astype(np.float64)
        new = update(i, x, eps, x0_prev, 0.0)
        x0_prev = (x - np.sqrt(1 - P.abar(i)) * eps) / np.sqrt(P.abar(i))
        a_p = P.abar(i + 1)
        k = np.sqrt(a_p) * known[0].astype(np.float64) + np.sqrt(1 - a_p) * z[0].astype(np.float64)
        x = M * new + (1 - M) * k
    assert_close(out, x[None].astype(np.float32), TOL_MODEL, TOL_MODEL_MAX, f"masked session 3 steps {kind}")


# ---- 8. state machine --------------------------------------------------------------------------------------------------------------------
def test_state_machine(gpu_ctx, tsd_mod, diffusion):
    from tsd._lib import TSD_E_ARG, TSD_E_STATE, TSD_OK, ptr
    lib = tsd_mod._lib.lib()
    B, L, steps = 1, 8, 4
    sampler = ("dpmpp_2m", 0.0, "trailing")
    lat, ctx, _, known, z = _inputs(B, L, tag=1190)
    mask = _mixed_mask(B, L)

    def loop(s, first=0):
        out = []
        for i in range(first, steps):
            s.step(i)
            out.append(s.latents())
        return np.stack(out)

    # before upload(): TSD_E_STATE - also after set_schedule / set_sampler, which invalidate the upload and the inpainting with it
    s = tsd_mod.Session(diffusion.model, None, B, L, 77, cfg=False)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, steps, 0)
    assert lib.tsd_session_set_inpaint(s.h, ptr(mask), ptr(known), ptr(z)) == TSD_E_STATE
    assert lib.tsd_session_inpaint_active(s.h) == 0
    s.upload(lat, ctx, None, None)
    unmasked = loop(s)
    s.upload(lat, ctx, None, None)
    s.set_inpaint(mask, known, z)
    assert s.inpaint_active
    masked = loop(s)
    assert not np.array_equal(masked[0], unmasked[0])
    s.set_schedule(N_TRAIN, steps, 0)
    assert not s.inpaint_active and lib.tsd_session_set_inpaint(s.h, ptr(mask), ptr(known), ptr(z)) == TSD_E_STATE

    # upload() turns it off: the next loop is the unmasked one
    s.upload(lat, ctx, None, None)
    s.set_inpaint(mask, known, z)
    s.upload(lat, ctx, None, None)
    assert not s.inpaint_active
    assert np.array_equal(_bits(loop(s)), _bits(unmasked))

    # set_inpaint(None) turns it off mid-loop: step 1 is then the unmasked step from the latents step 0 left (first order: the call
    # dropped the history, as an upload() of those latents does)
    s.upload(lat, ctx, None, None)
    s.set_inpaint(mask, known, z)
    s.step(0)
    assert np.array_equal(_bits(s.latents()), _bits(masked[0]))
    s.set_inpaint(None)
    assert not s.inpaint_active
    s.step(1)
    off = s.latents()
    s.upload(masked[0], ctx, None, None)
    s.step(1)
    assert np.array_equal(_bits(off), _bits(s.latents()))

    # refused arguments leave the state as it was - mask, tensors and history: the following steps are those of the run without them
    s.upload(lat, ctx, None, None)
    s.set_inpaint(mask, known, z)
    s.step(0)
    bad_known, bad_mask, bad_noise = known.copy(), mask.copy(), z.copy()
    bad_known[0, 1, 2, 3] = np.nan
    bad_mask[0, 4, 4] = 1.5
    bad_noise[0, 0, 0, 0] = np.inf
    other = np.ascontiguousarray(1.0 - mask)
    for m, k, n in ((other, bad_known, z), (bad_mask, known, z), (other, None, z), (other, known, bad_noise),
                    (np.full_like(mask, np.nan), known, z), (np.full_like(mask, -0.25), known, None)):
        assert lib.tsd_session_set_inpaint(s.h, ptr(m), ptr(k), ptr(n)) == TSD_E_ARG
        assert s.inpaint_active
    assert np.array_equal(_bits(loop(s, 1)), _bits(masked[1:]))

    # step(0), set_inpaint, step(1): the history was dropped, step 1 is the first-order host step and the blend
    s.upload(lat, ctx, None, None)
    s.step(0)
    assert np.array_equal(_bits(s.latents()), _bits(unmasked[0]))
    s.set_inpaint(mask, known, z)
    assert np.array_equal(_bits(s.latents()), _bits(unmasked[0]))     # the latents are not modified
    s.step(1)
    cd, second = (coeffs(tsd_mod, *sampler, steps, 1, h) for h in (0, 1))
    assert cd[6] == 0.0 and second[6] != 0.0
    x, _ = host_step(tsd_mod, gpu_ctx, diffusion, unmasked[0], ctx, None, 7.5, int(cd[0]), cd, None, None, False)
    x = blend_op(tsd_mod, gpu_ctx, x, mask, known, z, *blend_scalars(tsd_mod, *sampler, steps, 1))
    assert np.array_equal(_bits(s.latents()), _bits(x))

    # the Python shape checks
    for args in ((mask[:, :4], known, z), (mask, known[:, :3], z), (mask, known, z[:, :, :4]), (mask, None, z),
                 (np.ones((B, 2, L, L), np.float32), known, z)):
        with pytest.raises(ValueError):
            s.set_inpaint(*args)
    s.set_inpaint(mask[:, None], known)          # (B,1,L,L) and no noise are accepted
    assert s.inpaint_active
    assert lib.tsd_session_set_inpaint(s.h, None, None, None) == TSD_OK and not s.inpaint_active
    s.close()


# ---- 9. generate(mask=...) ---------------------------------------------------------------------------------------------------------------
def test_generate_with_a_mask(gpu_ctx, tsd_mod, diffusion, decoder, encoder):
    B, L, steps, strength, seed = 1, 8, 5, 0.6, 29
    nl = B * 4 * L * L
    _, ctx, _, _, _ = _inputs(B, L, tag=1200)
    image = rng.uniform(SEED, 1206, 3 * 64 * 64, 1.0).reshape(1, 3, 64, 64) * 127.5 + 127.5  # [0,255]
    mask = np.zeros((B, 1, 64, 64), dtype=np.float32)
    mask[:, :, 10:41, 20:50] = 1.0                # no multiple of 8: the `any` cells reach past it
    mask[:, :, 60, 3] = 0.6
    kw = dict(cfg=False, inference_steps=steps, seed_val=seed, L=L, input_image=image, encoder=encoder, strength=strength,
              sampler="dpmpp_2m", spacing="trailing", mask=mask)
    img = tsd_mod.generate(diffusion, decoder, ctx, **kw)
    assert img.shape == (B, 3, 64, 64) and np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 255.0
    lat = tsd_mod.generate(diffusion, decoder, ctx, return_latents=True, **kw)
    # the same by hand, with generate()'s RNG streams
    enc_lat = encoder.forward(tsd_mod.rescale(image, (0, 255), (-1, 1)), tsd_mod.rng.normal(seed, 1, nl).reshape(B, 4, L, L))
    mask_lat = tsd_mod.latent_mask(mask, "any")
    assert np.array_equal(mask_lat, latent_mask_np(mask[:, 0], MASK_ANY))
    assert mask_lat[0, 1:6, 2:7].all() and mask_lat[0, 7, 0] == 1 and mask_lat.sum() == 26
    z4 = tsd_mod.rng.normal(seed, 4, nl).reshape(B, 4, L, L)
    start = steps - int(steps * strength)
    s = _open(tsd_mod, diffusion.model, B, L, ("dpmpp_2m", 0.0, "trailing"), False, steps, enc_lat, ctx, None, start=start)
    assert s.num_steps == steps - start == 3
    s.add_noise(0, z4)
    s.set_inpaint(mask_lat, enc_lat, z4)
    for i in range(s.num_steps):
        s.step(i)
    assert np.array_equal(_bits(s.latents()), _bits(lat))
    s.close()
    keep = mask_per_element(mask_lat, lat.shape) == 0
    assert np.array_equal(_bits(lat)[keep], _bits(enc_lat)[keep])
    assert not np.array_equal(lat[~keep], enc_lat[~keep])
    assert not np.array_equal(lat, tsd_mod.generate(diffusion, decoder, ctx, return_latents=True, **dict(kw, mask=None)))
    with pytest.raises(ValueError):
        tsd_mod.generate(diffusion, decoder, ctx, **dict(kw, input_image=None))
    with pytest.raises(ValueError):
        tsd_mod.generate(diffusion, decoder, ctx, **dict(kw, mask=mask[:, :, :32]))


# ---- 10. launch accounting ---------------------------------------------------------------------------------------------------------------
LAUNCHES_PER_STEP = 161   # a step of the default (hoisted) session at B = 2, L = 8, any sampler, CFG on or off: measured on the parent commit


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=lambda s: s[0])
def test_a_masked_step_is_one_elementwise_launch_more(gpu_ctx, tsd_mod, diffusion, sampler, cfg):
    """Per-class launch counts of tsd_ctx_profile_begin / _end over 3 steady-state steps: with inpainting exactly one elementwise launch
    more per step, every other class unchanged; without it the count the session made before masked denoising existed."""
    B, L, steps, P = 2, 8, 4, 3
    lat, ctx, uctx, known, z = _inputs(B, L, tag=1210)

    def profile(masked):
        s = _open(tsd_mod, diffusion.model, B, L, sampler, cfg, steps, lat, ctx, uctx, _step_noise(B, L, steps, 1216))
        if masked:
            s.set_inpaint(_mixed_mask(B, L), known, z)
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
    print(f"[inpaint] {sampler[0]} cfg={cfg}: launches per step {sum(off.values()) // P} -> {sum(on.values()) // P}")
    assert sum(off.values()) == LAUNCHES_PER_STEP * P
    assert on["elementwise"] - off["elementwise"] == P
    assert {k: v for k, v in on.items() if k != "elementwise"} == {k: v for k, v in off.items() if k != "elementwise"}
