"""Helpers shared by test_gpu_inpaint.py and test_inpaint_cpu.py (test infrastructure): the raw C-ABI calls of the masked-denoising
entries, numpy restatements of the two kernels, and `coeffs` / `step_f32` / `host_step` restated from test_gpu_sampler.py."""
import ctypes as C

import numpy as np

from sampler_ref import N_TRAIN

KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}
SPACINGS = {"leading": 0, "trailing": 1}
MASK_AREA, MASK_ANY = 0, 1
U = 2.0 ** -24  # unit roundoff of fp32
NEW_ENTRIES = ("tsd_latent_mask_f32", "tsd_inpaint_blend_f32", "tsd_session_set_inpaint", "tsd_session_inpaint_active")


def coeffs(tsd_mod, kind, eta, spacing, n, i, have_history, start=0):
    out = (C.c_double * 8)()
    rc = tsd_mod._lib.lib().tsd_sampler_coeffs(KINDS[kind], float(eta), SPACINGS[spacing], N_TRAIN, n, start, i, int(have_history), out)
    assert rc == 0, tsd_mod._lib.last_error()
    return np.array(out[:], dtype=np.float64)


def blend_scalars(tsd_mod, kind, eta, spacing, n, i, start=0):
    """(a_prev, s_prev) as float32 of the blend after step i of a list of n - start entries: out[2], out[3] of tsd_sampler_coeffs for
    step i + 1, (1, 0) after the last entry."""
    if i + 1 >= n - start:
        return np.float32(1.0), np.float32(0.0)
    cd = coeffs(tsd_mod, kind, eta, spacing, n, i + 1, 0, start)
    return np.float32(cd[2]), np.float32(cd[3])


def step_f32(tsd_mod, ctx, x, eps, eps_u, scale, hist, noise, c6, want_hist=True):
    """`tsd_sampler_step_f32` -> (x', x0 or None)."""
    from tsd._lib import check, f32, ptr
    x, eps = f32(x), f32(eps)
    eps_u, hist, noise = (None if a is None else f32(a) for a in (eps_u, hist, noise))
    c = f32(np.asarray(c6, dtype=np.float32))
    out = np.empty_like(x)
    hout = np.empty_like(x) if want_hist else None
    check(tsd_mod._lib.lib().tsd_sampler_step_f32(ctx.h, ptr(x), ptr(eps), ptr(eps_u), float(scale), ptr(hist), ptr(noise), x.size, ptr(c),
                                                  ptr(out), ptr(hout)))
    return out, hout


def host_step(tsd_mod, gpu_ctx, diffusion, x, ctx, uctx, cfg_scale, t, cd, hist, noise, keep_hist):
    """One step as the session does it, from the host: UNet on the device-computed time embedding, then the update kernel with
    tsd_sampler_coeffs' scalars."""
    B = x.shape[0]
    temb = np.repeat(tsd_mod.get_time_embedding(float(t)).reshape(1, 320), B, axis=0)
    e_c = diffusion.forward(x, ctx, temb)
    e_u = diffusion.forward(x, uctx, temb) if uctx is not None else None
    c = cd[2:].astype(np.float32)
    return step_f32(tsd_mod, gpu_ctx, x, e_c, e_u, cfg_scale, hist, noise if (noise is not None and c[5] != 0) else None, c, keep_hist)


def blend_raw(tsd_mod, ctx, x, mask, known, noise, a_prev, s_prev, alias=False):
    """`tsd_inpaint_blend_f32` -> (status, x_out).  alias: x_out is x (the op then blends in place on the device, as a session does)."""
    from tsd._lib import f32, ptr
    x, mask, known = f32(x), f32(mask), f32(known)
    noise = None if noise is None else f32(noise)
    B = x.shape[0]
    hw = x.size // (4 * B)
    assert mask.size == B * hw
    xin = x.copy()
    out = xin if alias else np.empty_like(x)
    rc = tsd_mod._lib.lib().tsd_inpaint_blend_f32(ctx.h if ctx is not None else None, ptr(xin), ptr(mask), ptr(known), ptr(noise), B, hw,
                                                  float(a_prev), float(s_prev), ptr(out))
    return rc, out


def blend_op(tsd_mod, ctx, x, mask, known, noise, a_prev, s_prev):
    rc, out = blend_raw(tsd_mod, ctx, x, mask, known, noise, a_prev, s_prev)
    assert rc == 0, tsd_mod._lib.last_error()
    return out


def latent_mask_raw(tsd_mod, ctx, mask_px, B, L, mode):
    from tsd._lib import f32, ptr
    m = f32(mask_px)
    out = np.empty((max(B, 0), max(L, 0), max(L, 0)), dtype=np.float32)
    rc = tsd_mod._lib.lib().tsd_latent_mask_f32(ctx.h if ctx is not None else None, ptr(m), B, L, mode, ptr(out))
    return rc, out


def known_f32(known, noise, a_prev, s_prev):
    """k = fl(fl(a known) + fl(s noise)) in numpy float32: one rounding per operation, as the kernel's (no fma in numpy)."""
    a, s = np.float32(a_prev), np.float32(s_prev)
    k = a * np.asarray(known, dtype=np.float32)
    if noise is not None:
        k = k + s * np.asarray(noise, dtype=np.float32)
    assert k.dtype == np.float32
    return k


def mask_per_element(mask, shape):
    """mask (B, ...) broadcast over the 4 channels of x (B, 4, ...)."""
    B = shape[0]
    return np.broadcast_to(np.asarray(mask).reshape(B, 1, -1), (B, 4, np.asarray(mask).size // B)).reshape(shape)


def blend_f64(x, mask, known, noise, a_prev, s_prev):
    """-> (reference, sum of the absolute terms) in float64, the scalars taken as the floats the kernel takes."""
    X, K = np.asarray(x, np.float64), np.asarray(known, np.float64)
    M = mask_per_element(mask, X.shape).astype(np.float64)
    a, s = np.float64(np.float32(a_prev)), np.float64(np.float32(s_prev))
    k, absk = a * K, np.abs(a * K)
    if noise is not None:
        Z = np.asarray(noise, np.float64)
        k, absk = k + s * Z, absk + np.abs(s * Z)
    return M * X + (1.0 - M) * k, np.abs(M * X) + np.abs(1.0 - M) * absk


def latent_mask_np(mask_px, mode):
    """numpy restatement: (B,8L,8L) -> (B,L,L) float64 mean of each 8x8 block (area) or the 0/1 threshold of its maximum (any)."""
    m = np.asarray(mask_px)
    B, S, _ = m.shape
    blocks = m.reshape(B, S // 8, 8, S // 8, 8).transpose(0, 1, 3, 2, 4).reshape(B, S // 8, S // 8, 64)
    if mode == MASK_ANY:
        return (blocks.max(axis=-1) >= np.float32(0.5)).astype(np.float32)
    return blocks.astype(np.float64).sum(axis=-1) / 64.0
