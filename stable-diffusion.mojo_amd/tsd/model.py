"""Device-resident models (`tsd_model`) and the denoise session (`tsd_session`)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, check_guidance_rescale, f32, latent_shape, lib, prediction_type, ptr, sampler_kind, timestep_spacing, vp

KINDS = {"diffusion": _lib.MODEL_DIFFUSION, "decoder": _lib.MODEL_DECODER, "encoder": _lib.MODEL_ENCODER,
         "clip": _lib.MODEL_CLIP, "diffusion_sd15": _lib.MODEL_DIFFUSION_SD15,
         "diffusion_sd15_torch": _lib.MODEL_DIFFUSION_SD15_TORCH, "clip_torch": _lib.MODEL_CLIP_TORCH,
         "decoder_torch": _lib.MODEL_DECODER_TORCH, "encoder_torch": _lib.MODEL_ENCODER_TORCH,
         "controlnet_sd15": _lib.MODEL_CONTROLNET_SD15, "controlnet_sd15_torch": _lib.MODEL_CONTROLNET_SD15_TORCH,
         "ip_adapter_sd15": _lib.MODEL_IP_ADAPTER_SD15, "clip_vision_h": _lib.MODEL_CLIP_VISION_H,
         "ip_adapter_plus_sd15": _lib.MODEL_IP_ADAPTER_PLUS_SD15,
         "diffusion_sd2": _lib.MODEL_DIFFUSION_SD2, "clip_sd2": _lib.MODEL_CLIP_SD2}


def param_specs(kind):
    """[(name, shape, used, init_bound)] in struct-field DFS order (SURVEY.md App.C).  No GPU needed."""
    k = KINDS[kind] if isinstance(kind, str) else kind
    n = lib().tsd_model_param_count(k)
    out = []
    name = C.create_string_buffer(128)
    shape = (C.c_int64 * 4)()
    ndim, used, bound = C.c_int(), C.c_int(), C.c_float()
    for i in range(n):
        check(lib().tsd_model_param_info(k, i, name, 128, shape, C.byref(ndim), C.byref(used), C.byref(bound)))
        out.append((name.value.decode(), tuple(int(shape[j]) for j in range(ndim.value)), bool(used.value), bound.value))
    return out


def flop_count(kind, L, T=77):
    """Algorithmic GFLOP of one forward per sample."""
    return lib().tsd_flop_count(KINDS[kind] if isinstance(kind, str) else kind, L, T)


class Model:
    """Packed device weights of Diffusion / Decoder / Encoder."""

    def __init__(self, kind, ctx=None, seed=None):
        self.kind = KINDS[kind] if isinstance(kind, str) else kind
        self.ctx = ctx or _lib.default_context()
        h = vp()
        check(lib().tsd_model_create(self.ctx.h, self.kind, C.byref(h)))
        self.h = h
        self.specs = param_specs(self.kind)
        if seed is not None:
            self.init_random(seed)

    def init_random(self, seed):
        check(lib().tsd_model_init_random(self.h, int(seed)))

    @property
    def context_width(self):
        """Width of the context rows a UNet / ControlNet reads and a text encoder writes (`tsd_model_context_width`): 768, or 1024 for the
        SD-2.x kinds."""
        w = lib().tsd_model_context_width(self.h)
        if w < 0:
            check(w)
        return w

    def set_param(self, index, array):
        a = f32(array)
        check(lib().tsd_model_set_param(self.h, int(index), ptr(a), a.size))

    def load_params(self, params):
        """params: {name: array} in the reference layouts (conv OIHW, linear (out,in))."""
        for i, (name, shape, used, _) in enumerate(self.specs):
            if name in params:
                self.set_param(i, np.asarray(params[name]).reshape(shape))
            elif used:
                raise KeyError(f"missing parameter {name}")

    def packed_blob(self):
        p, n = vp(), C.c_size_t()
        check(lib().tsd_model_packed_blob(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def mark_loaded(self):
        check(lib().tsd_model_mark_loaded(self.h))

    def prepare(self):
        """Build the derived device buffers now (per rank, after the weights are in place) and wait for them."""
        check(lib().tsd_model_prepare(self.h))

    def param_index(self, name_or_index):
        """Index of a parameter given its name (struct-field path, `param_specs`) or its index."""
        if isinstance(name_or_index, str):
            for i, spec in enumerate(self.specs):
                if spec[0] == name_or_index:
                    return i
            raise KeyError(f"no parameter {name_or_index}")
        i = int(name_or_index)
        if not 0 <= i < len(self.specs):
            raise IndexError(f"parameter index {i} out of range")
        return i

    def get_param(self, name_or_index):
        """The parameter as the forward reads it, in the reference layout (fp32 array): every weight is exactly an fp16 value (the
        device keeps no fp32 masters), biases and norm parameters are what was set."""
        i = self.param_index(name_or_index)
        out = np.empty(self.specs[i][1], dtype=np.float32)
        check(lib().tsd_model_get_param(self.h, i, ptr(out), out.size))
        return out

    def packed_param(self, name_or_index):
        """Raw packed bytes of the parameter (uint8 array; the device layout) - for tests of what a merge may touch."""
        i = self.param_index(name_or_index)
        n = lib().tsd_debug_model_packed_param(self.h, i, None, 0)
        if n < 0:
            check(n)
        out = np.empty(n, dtype=np.uint8)
        if n:
            r = lib().tsd_debug_model_packed_param(self.h, i, out.ctypes.data_as(vp), n)
            if r < 0:
                check(r)
        return out

    def lora_add(self, name_or_index, up, down, scale, row0=0):
        """Merge a low-rank adapter into rows [row0, row0 + up.shape[0]) of a weight, on the device: W <- rn16(W + scale * up @ down),
        fp32 product, one rounding to fp16.  up (rows, rank); down (rank, cols) or a conv-shaped (rank, I, k, k), flattened to the
        reference column order.  The first add on a parameter keeps its base bits for `lora_clear`; repeated adds stack, one rounding
        each."""
        i = self.param_index(name_or_index)
        u, d = f32(up), f32(down)
        u = u.reshape(u.shape[0], -1)
        d = np.ascontiguousarray(d.reshape(d.shape[0], -1))
        shape = self.specs[i][1]
        if u.shape[1] != d.shape[0]:
            raise ValueError(f"up {u.shape} and down {d.shape} do not share a rank")
        if len(shape) >= 2 and d.shape[1] != int(np.prod(shape[1:])):
            raise ValueError(f"{self.specs[i][0]}: down has {d.shape[1]} columns, the parameter {int(np.prod(shape[1:]))}")
        check(lib().tsd_model_lora_add(self.h, i, int(row0), u.shape[0], ptr(u), ptr(d), u.shape[1], float(scale)))

    def lora_clear(self):
        """Every parameter touched by `lora_add` back to its base, bit for bit."""
        check(lib().tsd_model_lora_clear(self.h))

    @property
    def lora_count(self):
        """Parameters that currently differ from their base."""
        return lib().tsd_model_lora_count(self.h)

    def close(self):
        if self.h:
            lib().tsd_model_destroy(self.h)
            self.h = None


def _context_error(what, want, got):
    """The message of a context whose shape a model cannot read; a wrong width names both widths (a 768-wide SD-1.x context handed to an
    SD-2.x UNet, or the reverse, would otherwise be read as too few / too many floats by the C side)."""
    msg = f"{what} must have shape {want}, got {got}"
    if len(got) and got[-1] != want[-1]:
        msg += f": this UNet reads a {want[-1]}-wide context, the one given is {got[-1]} wide"
    return msg


class Session:
    """Device-resident denoise loop (pipeline.mojo:57-127 + sampler.mojo).  L: the latent side, or a pair (LH, LW) for a rectangular
    session; `LH` / `LW` are the sides, `L` stays what the caller passed.  Where a method's text says L,L the tensor is LH,LW."""

    def __init__(self, diffusion, decoder, B, L, T=77, cfg=False):
        LH, LW = latent_shape(L)
        h = vp()
        check(lib().tsd_session_create_hw(diffusion.h, decoder.h if decoder is not None else None, B, LH, LW, T, 1 if cfg else 0,
                                          C.byref(h)))
        self.h, self.B, self.L, self.T, self.cfg = h, B, L, T, cfg
        self.LH, self.LW = LH, LW
        self.ctx = diffusion.ctx
        self.has_decoder = decoder is not None
        self.W = diffusion.context_width   # the C side reads T * W floats per context

    def set_schedule(self, num_training_steps=1000, num_inference_steps=50, start_step=0):
        check(lib().tsd_session_set_schedule(self.h, num_training_steps, num_inference_steps, start_step))

    def set_sampler(self, kind="ddpm", eta=0.0, spacing="leading"):
        """"ddpm" (the reference's, default) | "ddim" (eta = 0 deterministic) | "dpmpp_2m"; spacing "leading" | "trailing".
        Like set_schedule it invalidates the upload."""
        check(lib().tsd_session_set_sampler(self.h, sampler_kind(kind), float(eta), timestep_spacing(spacing)))

    def set_prediction(self, prediction="epsilon", zero_terminal_snr=False):
        """What the model output means, "epsilon" (default) | "v" (Salimans & Ho 2022; diffusers' "v_prediction" is accepted), and whether
        the session runs on the zero-terminal-SNR rescale of the alphas_cumprod table (Lin et al. 2023, algorithm 1).  Session
        configuration like set_sampler: it invalidates the upload and persists across uploads.  Epsilon-prediction on a timestep list
        that contains the terminal timestep of that table (trailing spacing) is refused."""
        check(lib().tsd_session_set_prediction(self.h, prediction_type(prediction), 1 if zero_terminal_snr else 0))

    @property
    def prediction(self):
        """(prediction, zero_terminal_snr) as set_prediction takes them."""
        p, z = C.c_int(0), C.c_int(0)
        check(lib().tsd_session_prediction(self.h, C.byref(p), C.byref(z)))
        return ("epsilon", "v")[p.value], bool(z.value)

    @property
    def num_steps(self):
        return lib().tsd_session_num_steps(self.h)

    def timestep(self, i):
        return lib().tsd_session_timestep(self.h, i)

    def upload(self, latents, context, uncond_context=None, noise=None, cfg_scale=7.5):
        la, cx = f32(latents), f32(context)
        uc = f32(uncond_context) if uncond_context is not None else None
        nz = f32(noise) if noise is not None else None
        # the C side reads exactly B*4*L*L / B*T*W / steps*B*4*L*L floats from these pointers: check the shapes here
        B, LH, LW, T, W = self.B, self.LH, self.LW, self.T, self.W
        if la.shape != (B, 4, LH, LW):
            raise ValueError(f"latents must have shape {(B, 4, LH, LW)}, got {la.shape}")
        if cx.shape != (B, T, W):
            raise ValueError(_context_error("context", (B, T, W), cx.shape))
        if self.cfg and uc is None:
            raise ValueError("a CFG session needs uncond_context")
        if uc is not None:
            if uc.ndim == 2:
                uc = uc[None]
            if uc.shape == (1, T, W) and B > 1:  # one shared negative prompt: broadcast it like Diffusion.forward does
                uc = np.ascontiguousarray(np.broadcast_to(uc, (B, T, W)))
            if uc.shape != (B, T, W):
                raise ValueError(_context_error("uncond_context", (B, T, W), uc.shape) + f" (or one shared {(T, W)} row)")
        if nz is not None and nz.shape != (self.num_steps, B, 4, LH, LW):
            raise ValueError(f"noise must have shape {(self.num_steps, B, 4, LH, LW)}, got {nz.shape}")
        check(lib().tsd_session_upload(self.h, ptr(la), ptr(cx), ptr(uc), ptr(nz), float(cfg_scale)))

    def step(self, i):
        check(lib().tsd_session_step(self.h, int(i)))

    def add_noise(self, i, noise):
        nz = f32(noise)
        if nz.size != self.B * 4 * self.LH * self.LW or (nz.ndim == 4 and nz.shape != (self.B, 4, self.LH, self.LW)):
            raise ValueError(f"noise must have shape {(self.B, 4, self.LH, self.LW)}, got {nz.shape}")
        check(lib().tsd_session_add_noise(self.h, int(i), ptr(nz)))

    def set_seeds(self, seeds):
        """Seeded device-side noise for the steps of the current upload(): `seeds` is a sequence of B ints (uint64), one per sample; None
        turns it off.  A DDPM / DDIM(eta > 0) step then draws its noise in the update kernel from stream 16 + i of the sample's seed -
        the same values wherever the sample sits in the batch.  Needs an upload() without a noise tensor; upload(), set_schedule() and
        set_sampler() turn it off."""
        if seeds is None:
            check(lib().tsd_session_set_seeds(self.h, None))
            return
        seeds = [int(v) for v in seeds]
        if len(seeds) != self.B:
            raise ValueError(f"seeds must have one entry per sample ({self.B}), got {len(seeds)}")
        if any(v < 0 or v >= 1 << 64 for v in seeds):
            raise ValueError("every seed must fit an unsigned 64-bit integer")
        check(lib().tsd_session_set_seeds(self.h, (C.c_uint64 * self.B)(*seeds)))

    @property
    def seeds_active(self):
        return lib().tsd_session_seeds_active(self.h) == 1

    def seed_latents(self):
        """Replace the latents by stream 2 of each sample's seed (after set_seeds)."""
        check(lib().tsd_session_seed_latents(self.h))

    def add_noise_seeded(self, i):
        """add_noise at timestep index i with stream 4 of each sample's seed, drawn on the device (after set_seeds)."""
        check(lib().tsd_session_add_noise_seeded(self.h, int(i)))

    def set_inpaint(self, mask, known=None, noise=None, seeded=False):
        """Masked denoising for the steps of the current upload(): mask (B,L,L) or (B,1,L,L) in [0,1], 1 = regenerate and 0 = keep
        `known` (B,4,L,L), the original latents, re-noised after every step with `noise` (B,4,L,L; None: a noiseless known region).
        seeded=True (after set_seeds, no `noise`): the noise is stream 4 of each sample's seed, drawn on the device.
        mask=None turns it off.  upload(), set_schedule() and set_sampler() turn it off as well."""
        if seeded and noise is not None:
            raise ValueError("set_inpaint(seeded=True) draws its noise on the device: pass no noise tensor")
        if mask is None:
            check(lib().tsd_session_set_inpaint(self.h, None, None, None))
            return
        B, LH, LW = self.B, self.LH, self.LW
        m = f32(mask)
        if m.shape == (B, 1, LH, LW):
            m = np.ascontiguousarray(m.reshape(B, LH, LW))
        if m.shape != (B, LH, LW):
            raise ValueError(f"mask must have shape {(B, LH, LW)} or {(B, 1, LH, LW)}, got {m.shape}")
        if known is None:
            raise ValueError("set_inpaint with a mask needs the known latents")
        kn = f32(known)
        if kn.shape != (B, 4, LH, LW):
            raise ValueError(f"known must have shape {(B, 4, LH, LW)}, got {kn.shape}")
        nz = f32(noise) if noise is not None else None
        if nz is not None and nz.shape != (B, 4, LH, LW):
            raise ValueError(f"noise must have shape {(B, 4, LH, LW)}, got {nz.shape}")
        if seeded:
            check(lib().tsd_session_set_inpaint_seeded(self.h, ptr(m), ptr(kn)))
            return
        check(lib().tsd_session_set_inpaint(self.h, ptr(m), ptr(kn), ptr(nz)))

    @property
    def inpaint_active(self):
        return lib().tsd_session_inpaint_active(self.h) == 1

    def set_guidance_rescale(self, phi):
        """Guidance rescale (Lin et al. 2023, eq. 15-16; diffusers' `guidance_rescale`) for the steps of the current upload(): phi in
        [0, 1], 0 = off.  Every step then scales each sample's cond and uncond eps by g = phi std(cond) / std(combined) + 1 - phi on the
        device before its update (`tsd.cfg_rescale` is the same launches on host tensors).  Needs a CFG session; upload(),
        set_schedule() and set_sampler() turn it off."""
        phi = check_guidance_rescale(phi, self.cfg)
        check(lib().tsd_session_set_guidance_rescale(self.h, phi))

    def set_control(self, cn, hint=None, scale=1.0, cond_only=False, first_step=0, last_step=None):
        """ControlNet for the steps first_step <= i <= last_step (None: to the end) of this lockstep session on a full-size UNet
        (`tsd_session_set_control`): cn a `tsd.ControlNet` on the same context (None turns control off), hint (3,8LH,8LW) or
        (B,3,8LH,8LW), scale one value for every sample; cond_only: under CFG the uncond half gets scale 0.  Call after upload(); the
        hint encoder runs here once and every step inside the window runs the ControlNet and the controlled UNet forward on the device.
        The control stays across upload()s until set_control(None)."""
        if cn is None:
            check(lib().tsd_session_set_control(self.h, None, None, 0.0, 0, 0, -1))
            return
        h = f32(hint) if hint is not None else None
        if h is not None and h.ndim == 3:
            h = np.repeat(h[None], self.B, axis=0) if self.B > 1 else h[None]
        if h is None or h.shape != (self.B, 3, 8 * self.LH, 8 * self.LW):
            raise ValueError(f"set_control: the hint must have shape (3, {8 * self.LH}, {8 * self.LW}) or ({self.B}, 3, {8 * self.LH}, "
                             f"{8 * self.LW}), got {None if hint is None else np.shape(hint)}")
        h = f32(h)
        model = getattr(cn, "model", cn)
        check(lib().tsd_session_set_control(self.h, model.h, ptr(h), float(scale), 1 if cond_only else 0, int(first_step),
                                            -1 if last_step is None else int(last_step)))

    @property
    def control_active(self):
        return lib().tsd_session_control_active(self.h) == 1

    def set_ip_adapter(self, ip, tokens=None, uncond_tokens=None, scale=1.0, first_step=0, last_step=None):
        """IP-Adapter for the steps first_step <= i <= last_step (None: to the end) of this lockstep session on a full-size SD-1.x UNet
        (`tsd_session_set_ip_adapter`): ip a `tsd.IPAdapter` on the same context (None turns it off), tokens (N,768) or (B,N,768) for the
        conditional half and, in a CFG session, uncond_tokens of the same shape for the unconditional half - `ip.project(zeros)`, which
        is not zero tokens; scale one value for every sample.  Call after upload(); the keys and values of all blocks are projected here
        once, and the adapter stays across upload()s until set_ip_adapter(None)."""
        if ip is None:
            check(lib().tsd_session_set_ip_adapter(self.h, None, None, None, 0, 0.0, 0, -1))
            return

        def shaped(t, what):
            t = f32(t)
            if t.ndim == 2:
                t = np.repeat(t[None], self.B, axis=0) if self.B > 1 else t[None]
            if t.ndim != 3 or t.shape[0] != self.B or not (1 <= t.shape[1] <= 16) or t.shape[2] != 768:
                raise ValueError(f"set_ip_adapter: {what} must have shape (N, 768) or ({self.B}, N, 768) with 1 <= N <= 16, got {t.shape}")
            return f32(t)
        if tokens is None:
            raise ValueError("set_ip_adapter: the image tokens are required (IPAdapter.project(image_embeds))")
        tok = shaped(tokens, "tokens")
        unc = None
        if self.cfg:
            if uncond_tokens is None:
                raise ValueError("set_ip_adapter: a CFG session needs uncond_tokens (ip.project(zeros))")
            unc = shaped(uncond_tokens, "uncond_tokens")
            if unc.shape != tok.shape:
                raise ValueError(f"set_ip_adapter: tokens {tok.shape} and uncond_tokens {unc.shape} differ in shape")
        model = getattr(ip, "model", ip)
        check(lib().tsd_session_set_ip_adapter(self.h, model.h, ptr(tok), ptr(unc) if unc is not None else None, tok.shape[1], float(scale),
                                               int(first_step), -1 if last_step is None else int(last_step)))

    @property
    def ip_adapter_active(self):
        return lib().tsd_session_ip_adapter_active(self.h) == 1

    @property
    def guidance_rescale(self):
        phi = C.c_float(0.0)
        check(lib().tsd_session_guidance_rescale(self.h, C.byref(phi)))
        return phi.value

    def decode(self):
        check(lib().tsd_session_decode(self.h))

    def latents(self):
        out = np.empty((self.B, 4, self.LH, self.LW), dtype=np.float32)
        check(lib().tsd_session_download_latents(self.h, ptr(out)))
        return out

    def images(self, rescale=True):
        out = np.empty((self.B, 3, 8 * self.LH, 8 * self.LW), dtype=np.float32)
        check(lib().tsd_session_download_images(self.h, 1 if rescale else 0, ptr(out)))
        return out

    # ---- slot mode: every sample its own request, schedule index and guidance scale (tsd.h "slot sessions"; tsd/serve.py drives it) ----
    SLOT_IDLE, SLOT_ACTIVE, SLOT_DONE = 0, 1, 2

    def slots_open(self):
        """Enter slot mode, after set_sampler / set_schedule and in place of upload(): all B slots idle.  upload(), set_schedule() and
        set_sampler() leave it; the lockstep calls (step, set_seeds, decode, latents, ...) are refused while it is on."""
        check(lib().tsd_session_slots_open(self.h))

    def slot_start(self, b, context, uncond_context=None, latents=None, noise_at_start=False, seed=0, start_index=0, cfg_scale=7.5):
        """Put a request into slot b: context (T,768), uncond_context (T,768) on a CFG session, latents (4,L,L) or None (stream 2 of
        `seed`); noise_at_start noises given latents to timesteps[start_index] with stream 4 of `seed` (img2img)."""
        T, LH, LW, W = self.T, self.LH, self.LW, self.W
        cx = f32(context)
        if cx.shape == (1, T, W):
            cx = cx[0]
        if cx.shape != (T, W):
            raise ValueError(_context_error("context", (T, W), cx.shape))
        uc = None
        if uncond_context is not None:
            uc = f32(uncond_context)
            if uc.shape == (1, T, W):
                uc = uc[0]
            if uc.shape != (T, W):
                raise ValueError(_context_error("uncond_context", (T, W), uc.shape))
        la = None
        if latents is not None:
            la = f32(latents)
            if la.shape == (1, 4, LH, LW):
                la = la[0]
            if la.shape != (4, LH, LW):
                raise ValueError(f"latents must have shape {(4, LH, LW)}, got {la.shape}")
        seed = int(seed)
        if seed < 0 or seed >= 1 << 64:
            raise ValueError("the seed must fit an unsigned 64-bit integer")
        check(lib().tsd_session_slot_start(self.h, int(b), ptr(cx), ptr(uc), ptr(la), 1 if noise_at_start else 0, seed, int(start_index),
                                           float(cfg_scale)))

    def slot_set_inpaint(self, b, mask, known=None):
        """Masked denoising for the request of active slot b: mask (L,L) or (1,L,L) in [0,1], 1 = regenerate and 0 = keep `known`
        (4,L,L), the original latents, re-noised after every step with stream 4 of the slot's seed.  mask=None turns it off;
        slot_start() and slots_open() turn it off as well."""
        if mask is None:
            check(lib().tsd_session_slot_set_inpaint(self.h, int(b), None, None))
            return
        LH, LW = self.LH, self.LW
        m = f32(mask)
        if m.shape == (1, LH, LW):
            m = np.ascontiguousarray(m[0])
        if m.shape != (LH, LW):
            raise ValueError(f"mask must have shape {(LH, LW)} or {(1, LH, LW)}, got {m.shape}")
        if known is None:
            raise ValueError("slot_set_inpaint with a mask needs the known latents")
        kn = f32(known)
        if kn.shape == (1, 4, LH, LW):
            kn = np.ascontiguousarray(kn[0])
        if kn.shape != (4, LH, LW):
            raise ValueError(f"known must have shape {(4, LH, LW)}, got {kn.shape}")
        check(lib().tsd_session_slot_set_inpaint(self.h, int(b), ptr(m), ptr(kn)))

    def slot_inpaint_active(self, b):
        r = lib().tsd_session_slot_inpaint_active(self.h, int(b))
        if r < 0:
            check(r)
        return r == 1

    def slot_set_guidance_rescale(self, b, phi):
        """Guidance rescale for the request of active slot b, per request like cfg_scale: phi in [0, 1], 0 = off.  slot_start() and
        slots_open() clear it."""
        phi = check_guidance_rescale(phi, self.cfg)
        check(lib().tsd_session_slot_set_guidance_rescale(self.h, int(b), phi))

    def slot_guidance_rescale(self, b):
        phi = C.c_float(0.0)
        check(lib().tsd_session_slot_guidance_rescale(self.h, int(b), C.byref(phi)))
        return phi.value

    def advance(self):
        """One tick: one forward over all slots, every active slot one step further.  Returns the slots that finished (ascending)."""
        mask = C.c_uint32(0)
        check(lib().tsd_session_advance(self.h, C.byref(mask)))
        return [b for b in range(self.B) if mask.value >> b & 1]

    def slot_state(self, b):
        """(next schedule index, state) of slot b; state is SLOT_IDLE / SLOT_ACTIVE / SLOT_DONE."""
        idx, st = C.c_int(0), C.c_int(0)
        check(lib().tsd_session_slot_state(self.h, int(b), C.byref(idx), C.byref(st)))
        return idx.value, st.value

    def slot_latents(self, b):
        out = np.empty((4, self.LH, self.LW), dtype=np.float32)
        check(lib().tsd_session_slot_download(self.h, int(b), ptr(out)))
        return out

    def slots_active(self):
        n = lib().tsd_session_slots_active(self.h)
        if n < 0:
            check(n)
        return n

    def raw_latents(self):
        """The device's latent buffer (B,4,L,L) as it is, in any mode and unchecked (tsd_debug_session_latents; for tests)."""
        out = np.empty((self.B, 4, self.LH, self.LW), dtype=np.float32)
        check(lib().tsd_debug_session_latents(self.h, ptr(out)))
        return out

    def hoist_info(self):
        """{active, time_table, ctx_k, ctx_vt (device addresses), bytes, builds} of the step-invariant buffers (tsd_debug_session_hoist_info)."""
        info = (C.c_int64 * 6)()
        check(lib().tsd_debug_session_hoist_info(self.h, info))
        return dict(zip(("active", "time_table", "ctx_k", "ctx_vt", "bytes", "builds"), (int(v) for v in info)))

    def close(self):
        if self.h:
            lib().tsd_session_destroy(self.h)
            self.h = None
