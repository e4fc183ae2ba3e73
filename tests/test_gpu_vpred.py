"""GPU tests of v-prediction and the zero-terminal-SNR schedule: the v update kernels against fp64 with a forward error bound and
against the eps kernel (bitwise, where the arithmetic is the same sequence), the device session against a host-driven loop over the same
kernel (bitwise, terminal step included), against the oracle UNet driven by the fp64 restatement (tests/vpred_ref.py), with guidance
rescale, in slot mode against lockstep sessions, at the terminal index of add_noise and the inpainting blend, on rectangular latents,
the state machine, and the untouched default.  Tiny-SD at random init (seed 1234): its output is simply READ as v - the update, not the
model, is under test.  B = 2, L = 8, 4 steps unless said otherwise."""
import ctypes as C

import numpy as np
import pytest

import vpred_ref as R
from oracle import models, ops, rng
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, randn

pytestmark = pytest.mark.gpu
SEED = 1234
N_TRAIN = R.N_TRAIN
KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}
SPACINGS = {"leading": 0, "trailing": 1}
EPS, V = 0, 1
U = 2.0 ** -24  # unit roundoff of fp32
T = 77


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def coeffs(tsd_mod, kind, eta, spacing, n, i, have_history, pred=V, ztsnr=1, start=0):
    out = (C.c_double * 8)()
    rc = tsd_mod._lib.lib().tsd_sampler_coeffs_ex(KINDS[kind], float(eta), SPACINGS[spacing], N_TRAIN, n, start, i, int(have_history),
                                                  pred, int(ztsnr), out)
    assert rc == 0, tsd_mod._lib.last_error()
    return np.array(out[:], dtype=np.float64)


def raw_step(tsd_mod, ctx, name, x, v, c6):
    """The status code of tsd_sampler_step_v_f32 / tsd_sampler_step_f32 on (x, v) alone, nothing raised."""
    from tsd._lib import f32, ptr
    x, v, c = f32(x), f32(v), f32(np.asarray(c6, dtype=np.float32))
    out = np.empty_like(x)
    return getattr(tsd_mod._lib.lib(), name)(ctx.h, ptr(x), ptr(v), None, 1.0, None, None, x.size, ptr(c), ptr(out), None)


def eps_step(tsd_mod, ctx, x, e, e_u, scale, hist, noise, c6):
    """x_out of `tsd_sampler_step_f32` (the eps kernel)."""
    from tsd._lib import check, f32, ptr
    x, e = f32(x), f32(e)
    e_u, hist, noise = (None if a is None else f32(a) for a in (e_u, hist, noise))
    c = f32(np.asarray(c6, dtype=np.float32))
    out = np.empty_like(x)
    check(tsd_mod._lib.lib().tsd_sampler_step_f32(ctx.h, ptr(x), ptr(e), ptr(e_u), float(scale), ptr(hist), ptr(noise), x.size, ptr(c),
                                                  ptr(out), None))
    return out


def _inputs(B, L, tag):
    LH, LW = (L, L) if isinstance(L, int) else L
    lat = rng.normal(SEED, tag, B * 4 * LH * LW).reshape(B, 4, LH, LW)
    ctx = rng.normal(SEED, tag + 1, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(SEED, tag + 2, B * T * 768).reshape(B, T, 768)
    return lat, ctx, uctx


def _open(tsd_mod, model, B, L, sampler, cfg, steps, pred="v", ztsnr=True, start=0):
    s = tsd_mod.Session(model, None, B, L, T, cfg=cfg)
    s.set_prediction(pred, ztsnr)
    s.set_sampler(*sampler)
    s.set_schedule(N_TRAIN, steps, start)
    return s


# ---- 1. the kernel against fp64, element-wise ---------------------------------------------------------------------------------------
# (kind, eta, spacing, n, i, have_history): mid-schedule steps, and step 0 of a trailing list on the zero-terminal-SNR table = the terminal one
KERNEL_STEPS = [("ddpm", 0.0, "trailing", 20, 7, 0), ("ddim", 0.5, "trailing", 20, 9, 0), ("dpmpp_2m", 0.0, "trailing", 20, 7, 1),
                ("ddpm", 0.0, "trailing", 20, 0, 0), ("ddim", 0.5, "trailing", 4, 0, 0), ("dpmpp_2m", 0.0, "trailing", 4, 0, 0)]


@pytest.mark.parametrize("kind,eta,spacing,n,i,hist", KERNEL_STEPS)
def test_kernel_matches_fp64_within_the_forward_error_bound(gpu_ctx, tsd_mod, kind, eta, spacing, n, i, hist):
    """x' = c_x x + c_v v + c_h h + c_n z and h' = alpha_t x - sigma_t v, v = (v_c - v_u) s + v_u, with the float scalars of a real step
    on the zero-terminal-SNR table, for all 16 combinations of the optional pointers, at a length that is no multiple of the 256-thread
    block (274 blocks).

    Bound (forward error of a fixed sequence of fp32 operations, each one rounding, 2^-24 relative): k 2^-24 sum |term|, with
    absV = (|v_c| + |v_u|)(s + 1) in place of |v| under CFG, and k the roundings on the longest path, counted from
    sampler_step_v_element's source (fma contraction is off there):
      x': v = sub, mul, add (3) -> c_v * v (4) -> + c_x x (5) -> + c_h h (6) -> + c_n z (7)            k = 7
      h': v (3) -> sigma_t * v (4) -> alpha_t x - . (5)                                                k = 5, terms |alpha_t x| + sigma_t absV
    The fp64 side takes the float scalars as the kernel does, so the bound has no term for them.  At the terminal scalars (alpha_t = 0,
    sigma_t = 1) h' is 0 * x - 1 * v: the combined v with its sign flipped, bit for bit, where the eps kernel would store 0 / 0."""
    cd = coeffs(tsd_mod, kind, eta, spacing, n, i, hist)
    c = cd[2:].astype(np.float32)
    al, sg, c_x, c_v, c_h, c_n = (np.float64(v) for v in c)
    terminal = i == 0
    assert (al == 0.0 and sg == 1.0) == terminal
    nel = 70001
    x, v_c, v_u, h, z = (randn(1820 + k, nel).astype(np.float32) for k in range(5))
    scale = np.float32(7.5)
    worst = [0.0, 0.0]
    for mask in range(16):
        use_u, use_h, use_z, want_hist = (bool(mask >> b & 1) for b in range(4))
        got, got_h = tsd_mod.sampler_step_v(x, v_c, v_u if use_u else None, scale, h if use_h else None, z if use_z else None, c,
                                            want_hist, ctx=gpu_ctx)
        X, VC, VU, H, Z = (a.astype(np.float64) for a in (x, v_c, v_u, h, z))
        if use_u:
            Vv, absV = (VC - VU) * np.float64(scale) + VU, (np.abs(VC) + np.abs(VU)) * (np.float64(scale) + 1.0)
        else:
            Vv, absV = VC, np.abs(VC)
        ref = c_x * X + c_v * Vv
        terms = np.abs(c_x * X) + np.abs(c_v) * absV
        if use_h:
            ref, terms = ref + c_h * H, terms + np.abs(c_h * H)
        if use_z:
            ref, terms = ref + c_n * Z, terms + np.abs(c_n * Z)
        ratio = (np.abs(got.astype(np.float64) - ref) / (7 * U * terms)).max()
        worst[0] = max(worst[0], ratio)
        assert ratio <= 1.0, (kind, mask, ratio)
        if want_hist:
            ref0 = al * X - sg * Vv
            r0 = (np.abs(got_h.astype(np.float64) - ref0) / (5 * U * (np.abs(al * X) + sg * absV))).max()
            worst[1] = max(worst[1], r0)
            assert r0 <= 1.0, (kind, mask, r0)
            if terminal:
                combined = ((v_c - v_u) * scale + v_u) if use_u else v_c     # the kernel's own three fp32 roundings
                assert _same(got_h, -combined.astype(np.float32)), (kind, mask)
        else:
            assert got_h is None
    print(f"[vpred] kernel {kind} eta={eta} step {i}/{n}: worst error / bound  x' {worst[0]:.3f}  h' {worst[1]:.3f}")


# ---- 2. x' is the eps kernel's arithmetic ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,eta,i,hist", [("ddim", 0.5, 9, 0), ("dpmpp_2m", 0.0, 7, 1), ("dpmpp_2m", 0.0, 0, 0)])
def test_x_out_is_pinned_to_the_eps_kernel(gpu_ctx, tsd_mod, kind, eta, i, hist):
    """With the same c[2..5] the two kernels run the same sequence of fp32 operations for x': bitwise equal, with every combination of
    the optional inputs - whatever alpha_t and sigma_t are (they reach the history store only)."""
    c = coeffs(tsd_mod, kind, eta, "trailing", 20, i, hist)[2:].astype(np.float32)
    nel = 70001
    x, a, b, h, z = (randn(1830 + k, nel).astype(np.float32) for k in range(5))
    for mask in range(8):
        use_u, use_h, use_z = (bool(mask >> k & 1) for k in range(3))
        args = (x, a, b if use_u else None, 7.5, h if use_h else None, z if use_z else None, c)
        got, _ = tsd_mod.sampler_step_v(*args, want_hist=False, ctx=gpu_ctx)
        assert _same(got, eps_step(tsd_mod, gpu_ctx, *args)), (kind, mask)


# ---- 3. non-finite v is counted --------------------------------------------------------------------------------------------------------
def test_kernel_counts_non_finite_outputs(gpu_ctx, tsd_mod):
    from tsd._lib import TSD_E_NONFINITE, TSD_OK
    lib = tsd_mod._lib.lib()
    c = coeffs(tsd_mod, "ddim", 0.0, "trailing", 20, 5, 0)[2:]
    x, v = (randn(1840 + k, 1000).astype(np.float32) for k in range(2))
    assert lib.tsd_debug_nonfinite_count(gpu_ctx.h, 1) >= 0
    bad = v.copy()
    bad[[3, 500, 999]] = [np.inf, np.nan, -np.inf]
    assert raw_step(tsd_mod, gpu_ctx, "tsd_sampler_step_v_f32", x, bad, c) == TSD_E_NONFINITE   # the count, reported (and cleared)
    assert lib.tsd_debug_nonfinite_count(gpu_ctx.h, 0) == 0
    assert raw_step(tsd_mod, gpu_ctx, "tsd_sampler_step_v_f32", x, v, c) == TSD_OK


# ---- 4. session == host-driven loop ---------------------------------------------------------------------------------------------------
def host_step(tsd_mod, gpu_ctx, diffusion, x, ctx, uctx, cfg_scale, t, cd, hist, noise, keep_hist, phi=0.0):
    """One step as the session does it, from the host: UNet on the device-computed time embedding, its output read as v, [guidance
    rescale,] then the v update kernel with tsd_sampler_coeffs_ex' scalars rounded to float.  Noise where the plan takes it: c_n != 0."""
    B = x.shape[0]
    temb = np.repeat(tsd_mod.get_time_embedding(float(t)).reshape(1, 320), B, axis=0)
    v_c = diffusion.forward(x, ctx, temb)
    v_u = diffusion.forward(x, uctx, temb) if uctx is not None else None
    if phi > 0.0:
        v_c, v_u, _ = tsd_mod.cfg_rescale(v_c, v_u, cfg_scale, phi, ctx=gpu_ctx)
    c = cd[2:].astype(np.float32)
    return tsd_mod.sampler_step_v(x, v_c, v_u, cfg_scale, hist, noise if (noise is not None and c[5] != 0) else None, c, keep_hist,
                                  ctx=gpu_ctx)


def run_both(tsd_mod, gpu_ctx, diffusion, B, L, sampler, cfg, steps, tag, pred="v", ztsnr=True, noise="upload", phi=0.0, seeds=None):
    """The session's latents after every step against the host loop's, bitwise.  noise "upload": a host tensor; "seeded": set_seeds on the
    device against tsd_normal_fill_f32's stream 16 + i of each sample's seed uploaded by the host loop."""
    kind, eta, spacing = sampler
    lat, ctx, uctx = _inputs(B, L, tag)
    chw = lat[0].size
    nz = rng.normal(SEED, tag + 3, steps * lat.size).reshape((steps,) + lat.shape)
    s = _open(tsd_mod, diffusion.model, B, L, sampler, cfg, steps, pred, ztsnr)
    s.upload(lat, ctx, uctx if cfg else None, nz if noise == "upload" else None, cfg_scale=7.5)
    if noise == "seeded":
        s.set_seeds(seeds)
        nz = np.stack([np.stack([tsd_mod.normal_fill(sd, 16 + i, chw, ctx=gpu_ctx).reshape(lat[0].shape) for sd in seeds])
                       for i in range(steps)])
    if phi > 0.0:
        s.set_guidance_rescale(phi)
    x, hist = lat, None
    multistep = kind == "dpmpp_2m"
    p = tsd_mod._lib.PREDICTION_TYPES[pred]
    took_noise = 0
    for i in range(steps):
        s.step(i)
        got = s.latents()
        cd = coeffs(tsd_mod, kind, eta, spacing, steps, i, hist is not None, p, ztsnr)
        assert int(cd[0]) == s.timestep(i)
        if ztsnr and spacing == "trailing" and i == 0:
            assert cd[2] == 0.0 and cd[3] == 1.0          # the terminal step is part of the run
        took_noise += np.float32(cd[7]) != 0
        x, h = host_step(tsd_mod, gpu_ctx, diffusion, x, ctx, uctx if cfg else None, 7.5, int(cd[0]), cd, hist, nz[i], multistep, phi)
        hist = h if multistep else None
        assert np.isfinite(got).all()
        assert _same(got, x), (sampler, cfg, i, float(np.abs(got - x).max()))
    s.close()
    return took_noise


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("sampler", [("ddpm", 0.0, "trailing"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")], ids=lambda s: s[0])
def test_session_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, diffusion, sampler, cfg):
    """Zero-terminal-SNR table, trailing spacing: step 0 is the terminal one (alpha_t = 0).  The UNet is bitwise batch invariant and the
    update is the same kernel on the same scalars, so the session's latents after every step ARE the host loop's.  Under v a DDPM
    session is an LMS plan too, and takes noise on every step but the last."""
    took = run_both(tsd_mod, gpu_ctx, diffusion, 2, 8, sampler, cfg, 4, tag=1850)
    assert took == {"ddpm": 3, "ddim": 3, "dpmpp_2m": 0}[sampler[0]]


def test_session_equals_the_host_loop_on_the_plain_table(gpu_ctx, tsd_mod, diffusion):
    """v-prediction without the rescale (an SD-2.x-768-style model): plain table, leading spacing."""
    run_both(tsd_mod, gpu_ctx, diffusion, 2, 8, ("dpmpp_2m", 0.0, "leading"), True, 4, tag=1860, ztsnr=False)
    assert run_both(tsd_mod, gpu_ctx, diffusion, 2, 8, ("ddpm", 0.0, "leading"), False, 4, tag=1864, ztsnr=False) == 3


def test_seeded_session_equals_uploading_the_same_stream(gpu_ctx, tsd_mod, diffusion):
    """set_seeds: the v update draws its noise in the kernel (k_sampler_step_v_seeded) - the values tsd_normal_fill_f32 gives for stream
    16 + i of the sample's seed, which the host loop uploads."""
    assert run_both(tsd_mod, gpu_ctx, diffusion, 2, 8, ("ddim", 0.5, "trailing"), True, 4, tag=1870, noise="seeded", seeds=[1234567, 89]) == 3


# ---- 5. against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
def test_session_matches_the_oracle_loop(gpu_ctx, tsd_mod, diffusion, unet_params, kind):
    """4 steps of the device loop from pure noise at t = 999 against the oracle UNet (its output read as v) driven by the fp64
    restatement of the papers' updates on the restatement's own zero-terminal-SNR table (vpred_ref), at the bound
    test_gpu_sampler.test_session_matches_the_oracle_loop holds the eps session to: the error source is the same UNet.  4 steps, not
    its 3: the terminal step and the one after it are first order by definition, the last one returns x0, so the third is the
    only one on which DPM-Solver++(2M) runs second order."""
    B, L, steps = 1, 8, 4
    lat, ctx, _ = _inputs(B, L, tag=1880)
    s = _open(tsd_mod, diffusion.model, B, L, (kind, 0.0, "trailing"), False, steps)
    ts = [s.timestep(i) for i in range(s.num_steps)]
    assert ts == [999, 749, 499, 249]
    s.upload(lat, ctx, None, None)
    for i in range(steps):
        s.step(i)
    out = s.latents()
    s.close()
    P = R.VPapers(ts, R.table(N_TRAIN, True))
    update = P.update(kind, 0.0)
    x, x0_prev = lat[0].astype(np.float64), None
    for i, t in enumerate(ts):
        v = models.diffusion(unet_params, x.astype(np.float32), ctx[0], ops.time_embedding(float(t))).astype(np.float64)
        new = update(i, x, v, x0_prev, 0.0)
        x0_prev, _ = P.x0_eps(i, x, v)
        x = new
    assert_close(out, x[None].astype(np.float32), TOL_MODEL, TOL_MODEL_MAX, f"v session 4 steps {kind}")


# ---- 6. guidance rescale under v --------------------------------------------------------------------------------------------------------
def test_guidance_rescale_scales_v_like_the_host_loop(gpu_ctx, tsd_mod, diffusion):
    """set_guidance_rescale(0.7) is a pre-pass over the model output whatever it means: the session equals tsd_cfg_rescale_f32 followed
    by the v update, bitwise, with the history (the data prediction of the rescaled v) carried through."""
    run_both(tsd_mod, gpu_ctx, diffusion, 2, 8, ("dpmpp_2m", 0.0, "trailing"), True, 4, tag=1890, phi=0.7)


# ---- 7. slots ----------------------------------------------------------------------------------------------------------------------------
SB = 3   # slot sessions and their lockstep references: 3 samples, so that one slot can stay idle


def _request(k, L=8):
    return dict(ctx=rng.normal(SEED, 1900 + 10 * k, T * 768).reshape(T, 768), uctx=rng.normal(SEED, 1901 + 10 * k, T * 768).reshape(T, 768),
                seed=3000017 * (k + 1) + 5, scale=(7.5, 3.0)[k % 2], lat=rng.normal(SEED, 1902 + 10 * k, 4 * L * L).reshape(4, L, L).astype(np.float32))


def _mask(L=8):
    """0, 1 and fractions, distinct rows, not symmetric under transposition."""
    v = (np.arange(L * L).reshape(L, L) * 5 + 1) % 13
    return np.where(v < 4, 0.0, np.where(v > 9, 1.0, v / 16.0)).astype(np.float32)


def _lockstep(tsd_mod, model, sampler, k, pos, start, img2img, mask=None, steps=4, L=8):
    """Sample `pos` of a lockstep v / zero-terminal-SNR session of SB samples running request k there: txt2img (seed_latents) or img2img
    from index `start` (add_noise_seeded), with `mask` inpainting (set_inpaint seeded; all ones for the other samples)."""
    req = _request(k)
    lat, ctx, uctx = _inputs(SB, L, tag=1960)
    lat, ctx, uctx = lat.astype(np.float32).copy(), ctx.copy(), uctx.copy()
    lat[pos], ctx[pos], uctx[pos] = req["lat"], req["ctx"], req["uctx"]
    seeds = [91, 92, 93]
    seeds[pos] = req["seed"]
    s = _open(tsd_mod, model, SB, L, sampler, True, steps)
    s.upload(lat, ctx, uctx, None, cfg_scale=req["scale"])
    s.set_seeds(seeds)
    if img2img:
        s.add_noise_seeded(start)
    else:
        s.seed_latents()
    if mask is not None:
        masks = np.ones((SB, L, L), dtype=np.float32)
        masks[pos] = mask
        s.set_inpaint(masks, lat, seeded=True)
    for i in range(start, steps):
        s.step(i)
    out = s.latents()[pos].copy()
    s.close()
    return out


@pytest.mark.parametrize("sampler", [("ddpm", 0.0, "trailing"), ("dpmpp_2m", 0.0, "trailing")], ids=lambda s: s[0])
def test_staggered_slots_equal_lockstep_bitwise(gpu_ctx, tsd_mod, diffusion, sampler):
    """A v / zero-terminal-SNR slot session (k_slot_update_v): slot 0 starts at tick 0, slot 1 two ticks late - so an advance holds one
    slot at the terminal step next to one mid-schedule - and slot 2 stays idle and is never written.  Each slot's latents == the same
    sample of the lockstep session of its request, bit for bit."""
    steps = 4
    s = _open(tsd_mod, diffusion.model, SB, 8, sampler, True, steps)
    s.slots_open()
    assert s.prediction == ("v", True)
    finished = {}
    for tick in range(steps + 2):
        for b in ((0,) if tick == 0 else (1,) if tick == 2 else ()):
            req = _request(b)
            s.slot_start(b, req["ctx"], req["uctx"], seed=req["seed"], cfg_scale=req["scale"])
        for b in s.advance():
            finished[b] = (tick, s.slot_latents(b))
    raw = s.raw_latents()
    s.close()
    assert sorted(finished) == [0, 1] and finished[0][0] == steps - 1 and finished[1][0] == steps + 1
    assert not raw[2].any()                                   # the idle slot holds the zeros of slots_open
    for b in (0, 1):
        ref = _lockstep(tsd_mod, diffusion.model, sampler, b, b, 0, img2img=False)
        assert np.isfinite(finished[b][1]).all()
        assert _same(finished[b][1], ref), (b, float(np.abs(finished[b][1] - ref).max()))


@pytest.mark.parametrize("sampler", [("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")], ids=lambda s: s[0])
def test_img2img_and_inpainting_slots_equal_lockstep_bitwise(gpu_ctx, tsd_mod, diffusion, sampler):
    """Slot 0: img2img from index 1.  Slot 1: inpainting from index 0, the terminal index - its noise at the start replaces the latents
    (0 * x + 1 * z) and its known region is held at every step by the update launch that blends (k_slot_update_blend_v)."""
    steps = 4
    s = _open(tsd_mod, diffusion.model, SB, 8, sampler, True, steps)
    s.slots_open()
    r0, r1 = _request(0), _request(1)
    s.slot_start(0, r0["ctx"], r0["uctx"], latents=r0["lat"], noise_at_start=True, seed=r0["seed"], start_index=1, cfg_scale=r0["scale"])
    s.slot_start(1, r1["ctx"], r1["uctx"], latents=r1["lat"], noise_at_start=True, seed=r1["seed"], start_index=0, cfg_scale=r1["scale"])
    s.slot_set_inpaint(1, _mask(), r1["lat"])
    z = tsd_mod.normal_fill(r1["seed"], 4, 4 * 8 * 8, ctx=gpu_ctx).reshape(4, 8, 8)
    assert _same(s.raw_latents()[1], z)                       # at abar = 0 add_noise leaves exactly the noise
    got = {}
    for tick in range(steps):
        for b in s.advance():
            got[b] = s.slot_latents(b)
    raw = s.raw_latents()
    s.close()
    assert sorted(got) == [0, 1] and not raw[2].any()
    ref0 = _lockstep(tsd_mod, diffusion.model, sampler, 0, 0, 1, img2img=True)
    ref1 = _lockstep(tsd_mod, diffusion.model, sampler, 1, 1, 0, img2img=True, mask=_mask())
    assert _same(got[0], ref0), float(np.abs(got[0] - ref0).max())
    assert _same(got[1], ref1), float(np.abs(got[1] - ref1).max())
    keep = _mask() == 0.0
    assert keep.any() and _same(got[1][:, keep], r1["lat"][:, keep])   # the known region after the last step: known, bit for bit
    assert not _same(got[1], _lockstep(tsd_mod, diffusion.model, sampler, 1, 1, 0, img2img=True))   # the mask matters


# ---- 8. noise at the terminal index -----------------------------------------------------------------------------------------------------
def test_noise_at_the_terminal_index_and_the_known_region(gpu_ctx, tsd_mod, diffusion):
    """add_noise_seeded(0) on a trailing zero-terminal-SNR list is sqrt(0) x + sqrt(1) z: exactly the stream it draws.  With inpainting the
    known region is re-noised with the session's table after every step - all noise after step 0's predecessor, none after the last
    step: `known`, bit for bit."""
    B, L, steps = 2, 8, 4
    lat, ctx, uctx = _inputs(B, L, tag=1980)
    seeds = [424243, 17]
    s = _open(tsd_mod, diffusion.model, B, L, ("ddim", 0.0, "trailing"), True, steps)
    s.upload(lat, ctx, uctx, None, cfg_scale=7.5)
    s.set_seeds(seeds)
    s.add_noise_seeded(0)
    z = np.stack([tsd_mod.normal_fill(sd, 4, 4 * L * L, ctx=gpu_ctx).reshape(4, L, L) for sd in seeds])
    assert _same(s.latents(), z)
    z2 = rng.normal(SEED, 1984, lat.size).reshape(lat.shape).astype(np.float32)
    s.upload(lat, ctx, uctx, None, cfg_scale=7.5)
    s.add_noise(0, z2)                                        # the host-tensor entry reads the same table
    assert _same(s.latents(), z2)
    masks = np.stack([_mask(L), _mask(L).T.copy()])
    s.set_inpaint(masks, lat, z2)
    for i in range(steps):
        s.step(i)
    out = s.latents()
    s.close()
    keep = masks == 0.0
    for b in range(B):
        assert keep[b].any() and _same(out[b][:, keep[b]], lat[b].astype(np.float32)[:, keep[b]])
    assert np.isfinite(out).all()


# ---- 9. rectangular latents ----------------------------------------------------------------------------------------------------------------
def test_rectangular_session_equals_its_host_loop(gpu_ctx, tsd_mod, diffusion):
    run_both(tsd_mod, gpu_ctx, diffusion, 2, (8, 16), ("dpmpp_2m", 0.0, "trailing"), True, 4, tag=1990)


# ---- 10. state machine ---------------------------------------------------------------------------------------------------------------------
def test_state_machine(gpu_ctx, tsd_mod, diffusion):
    from tsd._lib import TSD_E_ARG, TSD_E_STATE
    lib = tsd_mod._lib.lib()
    B, L = 1, 8
    lat, ctx, _ = _inputs(B, L, tag=2000)
    s = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=False)
    assert s.prediction == ("epsilon", False)
    s.set_sampler("ddim", 0.0, "trailing")
    s.set_schedule(N_TRAIN, 3, 0)
    s.upload(lat, ctx, None, None)
    s.set_prediction("v", True)                  # after upload(): the table and the plans changed, the upload is stale
    assert s.prediction == ("v", True)
    with pytest.raises(tsd_mod.TsdError) as e:
        s.step(0)
    assert e.value.code == TSD_E_STATE
    s.upload(lat, ctx, None, None)
    s.step(0)
    s.upload(lat, ctx, None, None)               # it survives a second upload
    assert s.prediction == ("v", True)
    s.step(0)
    first = s.latents()
    assert np.isfinite(first).all()
    for pred, z in ((2, 0), (-1, 1), (1, 2), (0, -1)):
        assert lib.tsd_session_set_prediction(s.h, pred, z) == TSD_E_ARG, (pred, z)
    assert lib.tsd_session_set_prediction(s.h, EPS, 1) == TSD_E_ARG      # epsilon + the terminal timestep of this trailing list
    assert b"alpha_bar = 0" in lib.tsd_last_error()
    assert s.prediction == ("v", True)
    s.step(1)                                    # a refused call changed nothing: the upload is still valid
    with pytest.raises(tsd_mod.TsdError) as e:
        s.set_prediction("sample")
    assert e.value.code == TSD_E_ARG
    # the refusal comes from whichever call completes the combination
    s.set_sampler("ddim", 0.0, "leading")
    s.set_prediction("epsilon", True)            # fine: a leading list never holds N - 1
    assert lib.tsd_session_set_sampler(s.h, 1, 0.0, 1) == TSD_E_ARG       # ... trailing would
    assert lib.tsd_session_set_schedule(s.h, 1, 1, 0) == TSD_E_ARG        # a one-entry table has no rescale
    assert s.prediction == ("epsilon", True) and [s.timestep(i) for i in range(s.num_steps)] == [666, 333, 0]
    s.close()
    # img2img drops the terminal entry: epsilon on the rescaled table is allowed on a trailing list once the schedule starts past it
    s = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=False)
    s.set_prediction("epsilon", True)
    s.set_schedule(N_TRAIN, 4, 1)                # leading default, start 1
    s.set_sampler("ddim", 0.0, "trailing")       # trailing list without its first entry: no abar = 0 in it
    assert [s.timestep(i) for i in range(s.num_steps)] == [749, 499, 249]
    assert lib.tsd_session_set_schedule(s.h, N_TRAIN, 4, 0) == TSD_E_ARG  # set_schedule completes the combination
    s.upload(lat, ctx, None, None)
    s.step(0)
    assert np.isfinite(s.latents()).all()
    s.close()


# ---- 11. the default is untouched ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [("ddpm", 0.0, "leading"), ("dpmpp_2m", 0.0, "trailing")], ids=lambda s: s[0])
def test_default_session_is_unchanged(gpu_ctx, tsd_mod, diffusion, sampler):
    """A session on which set_prediction was never called and one with set_prediction("epsilon", False): the same bits after every step
    and the same launch records (class and shape of every launch, in order) - and other bits than the v session's, so the test can tell."""
    B, L, steps = 2, 8, 4
    lat, ctx, uctx = _inputs(B, L, tag=2010)
    noise = rng.normal(SEED, 2013, steps * lat.size).reshape((steps,) + lat.shape)
    runs = []
    for mode in ("never", "explicit", "v"):
        s = tsd_mod.Session(diffusion.model, None, B, L, T, cfg=True)
        if mode == "explicit":
            s.set_prediction("epsilon", False)
        if mode == "v":
            s.set_prediction("v", False)
        s.set_sampler(*sampler)
        s.set_schedule(N_TRAIN, steps, 0)
        s.upload(lat, ctx, uctx, noise, cfg_scale=7.5)
        per_step = []
        gpu_ctx.profile_begin()
        try:
            for i in range(steps):
                s.step(i)
                per_step.append(s.latents())
            recs = gpu_ctx.profile_records()
        finally:
            gpu_ctx.profile_end()
        s.close()
        runs.append((np.stack(per_step), [r[:5] for r in recs]))
    assert _same(runs[0][0], runs[1][0])
    assert len(runs[0][1]) > 100 and runs[0][1] == runs[1][1]
    assert not _same(runs[0][0][0], runs[2][0][0])
    assert len(runs[2][1]) == len(runs[0][1])    # and the v session makes as many launches
