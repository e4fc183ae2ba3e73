"""GPU tests of the DDIM / DPM-Solver++(2M) samplers: the update kernel against fp64 with a forward error bound, the device session
against a host-driven loop over the same kernel (bitwise), against the oracle UNet driven by the fp64 restatement of the papers
(tests/sampler_ref.py), the history rule and the state machine, img2img through `generate`, and the untouched default."""
import ctypes as C

import numpy as np
import pytest

from oracle import models, ops, rng, spec
from sampler_ref import N_TRAIN, Papers
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, randn

pytestmark = pytest.mark.gpu
SEED = 1234
KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}
SPACINGS = {"leading": 0, "trailing": 1}
U = 2.0 ** -24  # unit roundoff of fp32


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


@pytest.fixture(scope="module")
def decoder(gpu_ctx, tsd_mod):
    return tsd_mod.Decoder(seed=SEED)


def coeffs(tsd_mod, kind, eta, spacing, n, i, have_history, start=0):
    out = (C.c_double * 8)()
    rc = tsd_mod._lib.lib().tsd_sampler_coeffs(KINDS[kind], float(eta), SPACINGS[spacing], N_TRAIN, n, start, i, int(have_history), out)
    assert rc == 0, tsd_mod._lib.last_error()
    return np.array(out[:], dtype=np.float64)


def step_f32(tsd_mod, ctx, x, eps, eps_u, scale, hist, noise, c6, want_hist=True, raw=False):
    """`tsd_sampler_step_f32` -> (x', x0 or None); raw: -> the status code, nothing raised."""
    from tsd._lib import check, f32, ptr
    x, eps = f32(x), f32(eps)
    eps_u, hist, noise = (None if a is None else f32(a) for a in (eps_u, hist, noise))
    c = f32(np.asarray(c6, dtype=np.float32))
    out = np.empty_like(x)
    hout = np.empty_like(x) if want_hist else None
    rc = tsd_mod._lib.lib().tsd_sampler_step_f32(ctx.h, ptr(x), ptr(eps), ptr(eps_u), float(scale), ptr(hist), ptr(noise), x.size, ptr(c),
                                                 ptr(out), ptr(hout))
    if raw:
        return rc
    check(rc)
    return out, hout


def _inputs(B, L, T=77, tag=700):
    lat = rng.normal(SEED, tag, B * 4 * L * L).reshape(B, 4, L, L)
    ctx = rng.normal(SEED, tag + 1, B * T * 768).reshape(B, T, 768)
    return lat, ctx


# ---- 1. the kernel against fp64, element-wise ---------------------------------------------------------------------------------------
KERNEL_STEPS = [("ddpm", 1.0, "leading", 20, 5, 0), ("ddim", 0.0, "leading", 20, 5, 0), ("ddim", 0.5, "trailing", 20, 0, 0),
                ("dpmpp_2m", 0.0, "trailing", 20, 7, 1), ("dpmpp_2m", 0.0, "leading", 20, 19, 1), ("dpmpp_2m", 0.0, "trailing", 4, 1, 1)]


@pytest.mark.parametrize("kind,eta,spacing,n,i,hist", KERNEL_STEPS)
def test_kernel_matches_fp64_within_the_forward_error_bound(gpu_ctx, tsd_mod, kind, eta, spacing, n, i, hist):
    """x' = c_x x + c_e e + c_h h + c_n z and x0 = (x - sigma_t e) / alpha_t, e = (e_c - e_u) s + e_u, with the float scalars of a real
    schedule step, for every combination of the optional pointers, at a length that is no multiple of the 256-thread block.

    Bound (forward error of a fixed sequence of fp32 operations, each one rounding, 2^-24 relative): k 2^-24 sum |term|, where the
    terms are those of the result with (|e_c| + |e_u|)(s + 1) in place of |e| under CFG, and k the roundings on the longest path,
    counted from k_sampler_step's source (fma contraction is off there):
      x': e = sub, mul, add (3) -> c_e * e (4) -> + c_x x (5) -> + c_h h (6) -> + c_n z (7)            k = 7
      x0: e (3) -> sigma_t * e (4) -> x - . (5) -> / alpha_t (6, correctly rounded division)           k = 6
    The fp64 side takes the float scalars as the kernel does, so the bound has no term for them."""
    cd = coeffs(tsd_mod, kind, eta, spacing, n, i, hist)
    c = cd[2:].astype(np.float32)
    al, sg, c_x, c_e, c_h, c_n = (np.float64(v) for v in c)
    nel = 70001
    x, e_c, e_u, h, z = (randn(720 + k, nel).astype(np.float32) for k in range(5))
    scale = np.float32(7.5)
    worst = [0.0, 0.0]
    for mask in range(16):
        use_u, use_h, use_z, want_hist = (bool(mask >> b & 1) for b in range(4))
        got, got_h = step_f32(tsd_mod, gpu_ctx, x, e_c, e_u if use_u else None, scale, h if use_h else None, z if use_z else None, c,
                              want_hist)
        X, EC, EU, H, Z = (a.astype(np.float64) for a in (x, e_c, e_u, h, z))
        if use_u:
            E, absE = (EC - EU) * np.float64(scale) + EU, (np.abs(EC) + np.abs(EU)) * (np.float64(scale) + 1.0)
        else:
            E, absE = EC, np.abs(EC)
        ref = c_x * X + c_e * E
        terms = np.abs(c_x * X) + np.abs(c_e) * absE
        if use_h:
            ref, terms = ref + c_h * H, terms + np.abs(c_h * H)
        if use_z:
            ref, terms = ref + c_n * Z, terms + np.abs(c_n * Z)
        ratio = (np.abs(got.astype(np.float64) - ref) / (7 * U * terms)).max()
        worst[0] = max(worst[0], ratio)
        assert ratio <= 1.0, (kind, mask, ratio)
        if want_hist:
            ref0 = (X - sg * E) / al
            r0 = (np.abs(got_h.astype(np.float64) - ref0) / (6 * U * (np.abs(X) + sg * absE) / al)).max()
            worst[1] = max(worst[1], r0)
            assert r0 <= 1.0, (kind, mask, r0)
        else:
            assert got_h is None
    print(f"[sampler] kernel {kind} eta={eta} {spacing} step {i}/{n}: worst error / bound  x' {worst[0]:.3f}  x0 {worst[1]:.3f}")


def test_kernel_counts_non_finite_outputs(gpu_ctx, tsd_mod):
    from tsd._lib import TSD_E_NONFINITE, TSD_OK
    lib = tsd_mod._lib.lib()
    c = coeffs(tsd_mod, "ddim", 0.0, "leading", 20, 5, 0)[2:]
    x, eps = (randn(740 + k, 1000).astype(np.float32) for k in range(2))
    assert lib.tsd_debug_nonfinite_count(gpu_ctx.h, 1) >= 0
    bad = eps.copy()
    bad[[3, 500, 999]] = [np.inf, np.nan, -np.inf]
    assert step_f32(tsd_mod, gpu_ctx, x, bad, None, 1.0, None, None, c, raw=True) == TSD_E_NONFINITE   # the count, reported (and cleared)
    assert lib.tsd_debug_nonfinite_count(gpu_ctx.h, 0) == 0
    assert step_f32(tsd_mod, gpu_ctx, x, eps, None, 1.0, None, None, c, raw=True) == TSD_OK


# ---- 2. session == host-driven loop -------------------------------------------------------------------------------------------------
def host_step(tsd_mod, gpu_ctx, diffusion, x, ctx, uctx, cfg_scale, t, cd, hist, noise, keep_hist):
    """One step as the session does it, from the host: UNet on the device-computed time embedding (both routes see bit-identical
    inputs, as in test_cfg_batch_equals_two_passes), then the update kernel with tsd_sampler_coeffs' scalars."""
    B = x.shape[0]
    temb = np.repeat(tsd_mod.get_time_embedding(float(t)).reshape(1, 320), B, axis=0)
    e_c = diffusion.forward(x, ctx, temb)
    e_u = diffusion.forward(x, uctx, temb) if uctx is not None else None
    c = cd[2:].astype(np.float32)
    return step_f32(tsd_mod, gpu_ctx, x, e_c, e_u, cfg_scale, hist, noise if (noise is not None and c[5] != 0) else None, c, keep_hist)


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("kind,eta,spacing", [("ddim", 0.0, "leading"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")])
def test_session_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, diffusion, kind, eta, spacing, cfg):
    """The UNet is bitwise batch invariant (the CFG batch of 2B equals two passes of B) and the update is the same kernel on the same
    scalars - reading eps in the output convolution's layout in the session and CHW from the host, which changes no arithmetic - so
    the session's latents after every step ARE the host loop's."""
    B, L, steps = 2, 8, 4
    lat, ctx = _inputs(B, L, tag=750)
    _, uctx = _inputs(B, L, tag=760)
    noise = rng.normal(SEED, 770, steps * B * 4 * L * L).reshape(steps, B, 4, L, L)
    s = tsd_mod.Session(diffusion.model, None, B, L, 77, cfg=cfg)
    s.set_sampler(kind, eta, spacing)
    s.set_schedule(N_TRAIN, steps, 0)
    s.upload(lat, ctx, uctx if cfg else None, noise, cfg_scale=7.5)
    x, hist = lat, None
    multistep = kind == "dpmpp_2m"
    for i in range(steps):
        s.step(i)
        got = s.latents()
        cd = coeffs(tsd_mod, kind, eta, spacing, steps, i, hist is not None)
        assert int(cd[0]) == s.timestep(i)
        x, h = host_step(tsd_mod, gpu_ctx, diffusion, x, ctx, uctx if cfg else None, 7.5, int(cd[0]), cd, hist, noise[i], multistep)
        hist = h if multistep else None
        assert np.array_equal(got, x), (kind, cfg, i, float(np.abs(got - x).max()))
    s.close()


# ---- 3. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
def test_session_matches_the_oracle_loop(gpu_ctx, tsd_mod, diffusion, unet_params, kind):
    """3 steps of the device loop vs the oracle UNet driven by the fp64 restatement of the paper's update (sampler_ref.Papers), on the
    schedule of test_session_denoise_matches_oracle (666, 333, 0), at the project's full-model tolerance."""
    B, L, steps = 1, 8, 3
    lat, ctx = _inputs(B, L, tag=780)
    s = tsd_mod.Session(diffusion.model, None, B, L, 77, cfg=False)
    s.set_sampler(kind, 0.0, "leading")
    s.set_schedule(N_TRAIN, steps, 0)
    ts = [s.timestep(i) for i in range(s.num_steps)]
    assert ts == [666, 333, 0]
    s.upload(lat, ctx, None, None)
    for i in range(steps):
        s.step(i)
    out = s.latents()
    s.close()
    P = Papers(ts)
    update = P.ddim(0.0) if kind == "ddim" else P.dpmpp_2m
    x, x0_prev = lat[0].astype(np.float64), None
    for i, t in enumerate(ts):
        eps = models.diffusion(unet_params, x.astype(np.float32), ctx[0], ops.time_embedding(float(t))).astype(np.float64)
        new = update(i, x, eps, x0_prev, 0.0)
        x0_prev = (x - np.sqrt(1 - P.abar(i)) * eps) / np.sqrt(P.abar(i))
        x = new
    assert_close(out, x[None].astype(np.float32), TOL_MODEL, TOL_MODEL_MAX, f"session 3 steps {kind}")


# ---- 4. history rule and state machine ---------------------------------------------------------------------------------------------
def test_history_rule(gpu_ctx, tsd_mod, diffusion):
    """DPM-Solver++(2M) runs second order only when the previous call was step(i - 1) since the last upload() / add_noise(): an
    out-of-order step, a step after add_noise() and a step after upload() equal the host loop with have_history = 0."""
    B, L, steps = 1, 8, 5
    lat, ctx = _inputs(B, L, tag=790)
    z = rng.normal(SEED, 792, B * 4 * L * L).reshape(B, 4, L, L)
    s = tsd_mod.Session(diffusion.model, None, B, L, 77, cfg=False)
    s.set_sampler("dpmpp_2m", 0.0, "trailing")
    s.set_schedule(N_TRAIN, steps, 0)

    def first_order(i, x):
        cd = coeffs(tsd_mod, "dpmpp_2m", 0.0, "trailing", steps, i, 0)
        second = coeffs(tsd_mod, "dpmpp_2m", 0.0, "trailing", steps, i, 1)
        assert cd[6] == 0.0 and second[6] != 0.0 and second[4] != cd[4]   # the two orders differ at this step: the test can tell
        return host_step(tsd_mod, gpu_ctx, diffusion, x, ctx, None, 7.5, int(cd[0]), cd, None, None, False)[0]

    s.upload(lat, ctx, None, None)
    s.step(0)
    x0 = s.latents()
    s.step(2)                                    # out of order
    assert np.array_equal(s.latents(), first_order(2, x0))
    s.step(3)                                    # ... and in order again: second order from step 2's prediction
    assert not np.array_equal(s.latents(), first_order(3, first_order(2, x0)))

    s.upload(lat, ctx, None, None)
    s.step(0)
    s.add_noise(1, z)                            # drops the history
    x1 = s.latents()
    s.step(1)
    assert np.array_equal(s.latents(), first_order(1, x1))

    s.upload(lat, ctx, None, None)
    s.step(0)
    s.upload(x0, ctx, None, None)                # drops the history
    s.step(1)
    assert np.array_equal(s.latents(), first_order(1, x0))
    s.close()


def test_state_machine(gpu_ctx, tsd_mod, diffusion):
    from tsd._lib import TSD_E_ARG, TSD_E_STATE
    lib = tsd_mod._lib.lib()
    B, L = 1, 8
    lat, ctx = _inputs(B, L, tag=800)
    s = tsd_mod.Session(diffusion.model, None, B, L, 77, cfg=False)
    s.set_schedule(N_TRAIN, 3, 0)
    s.upload(lat, ctx, None, None)
    s.set_sampler("ddim", 0.0, "trailing")       # after upload(): the list changed, the upload is stale
    assert [s.timestep(i) for i in range(s.num_steps)] == [999, 666, 332]
    with pytest.raises(tsd_mod.TsdError) as e:
        s.step(0)
    assert e.value.code == TSD_E_STATE
    s.upload(lat, ctx, None, None)
    s.step(0)
    assert np.isfinite(s.latents()).all()
    for kind, eta, spacing in ((3, 0.0, 0), (-1, 0.0, 0), (1, 0.0, 2), (1, 0.0, -1), (1, -0.1, 0), (1, float("nan"), 0)):
        assert lib.tsd_session_set_sampler(s.h, kind, eta, spacing) == TSD_E_ARG, (kind, eta, spacing)
    s.step(1)                                    # a refused call changed nothing
    with pytest.raises(tsd_mod.TsdError) as e:
        s.set_sampler("heun")
    assert e.value.code == TSD_E_ARG
    s.close()


# ---- 5. img2img with a new sampler -------------------------------------------------------------------------------------------------
def test_img2img_with_dpmpp_2m(gpu_ctx, tsd_mod, diffusion, decoder):
    B, L, steps, strength, seed = 1, 8, 5, 0.6, 23
    nl = B * 4 * L * L
    _, ctx = _inputs(B, L, tag=810)
    image = rng.uniform(SEED, 812, 3 * 64 * 64, 1.0).reshape(1, 3, 64, 64) * 127.5 + 127.5  # [0,255]
    enc = tsd_mod.Encoder(seed=SEED)
    kw = dict(cfg=False, inference_steps=steps, seed_val=seed, L=L, input_image=image, encoder=enc, strength=strength,
              sampler="dpmpp_2m", spacing="trailing")
    img = tsd_mod.generate(diffusion, decoder, ctx, **kw)
    assert img.shape == (B, 3, 64, 64) and np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 255.0
    lat = tsd_mod.generate(diffusion, decoder, ctx, return_latents=True, **kw)
    # the same by hand, with generate()'s RNG streams
    x = enc.forward(tsd_mod.rescale(image, (0, 255), (-1, 1)), tsd_mod.rng.normal(seed, 1, nl).reshape(B, 4, L, L))
    enc.model.close()
    s = tsd_mod.Session(diffusion.model, None, B, L, 77, cfg=False)
    s.set_sampler("dpmpp_2m", 0.0, "trailing")
    start = steps - int(steps * strength)
    s.set_schedule(N_TRAIN, steps, start)
    assert s.num_steps == steps - start == 3
    s.upload(x, ctx, None, None)
    s.add_noise(0, tsd_mod.rng.normal(seed, 4, nl).reshape(B, 4, L, L))
    for i in range(s.num_steps):
        s.step(i)
    assert np.array_equal(s.latents(), lat)
    s.close()


# ---- 6. the default is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
def test_default_session_is_the_ddpm_session(gpu_ctx, tsd_mod, diffusion, cfg):
    """A session on which set_sampler was never called and one with set_sampler("ddpm", 0, "leading") give the same bits over a 5-step
    loop with noise (bench.py --dump-outputs holds the default against the parent commit's bits)."""
    B, L, steps = 2, 8, 5
    lat, ctx = _inputs(B, L, tag=820)
    _, uctx = _inputs(B, L, tag=830)
    noise = rng.normal(SEED, 840, steps * B * 4 * L * L).reshape(steps, B, 4, L, L)
    got = []
    for explicit in (False, True):
        s = tsd_mod.Session(diffusion.model, None, B, L, 77, cfg=cfg)
        if explicit:
            s.set_sampler("ddpm", 0.0, "leading")
        s.set_schedule(N_TRAIN, steps, 0)
        s.upload(lat, ctx, uctx if cfg else None, noise, cfg_scale=7.5)
        per_step = []
        for i in range(steps):
            s.step(i)
            per_step.append(s.latents())
        s.close()
        got.append(np.stack(per_step))
    assert np.array_equal(got[0], got[1])
    assert not np.array_equal(got[0][-1], got[0][-2])
