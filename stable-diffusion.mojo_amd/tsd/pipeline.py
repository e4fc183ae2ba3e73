"""Host-side mirror of `pipeline.generate` (pipeline.mojo:12-127): [tokenizer -> CLIP ->] sampler -> [encoder] ->
denoise loop (UNet x1 or x2 with CFG) -> decoder -> rescale.  The context embedding is normally an input (the
measured path starts there); `encode_prompts` is the reference's prompt front end (pipeline.mojo:31-54).  Batched
over independent prompts (the reference is batch 1; `pipeline.mojo:12` suggests exactly this batching)."""
import numpy as np

from . import rng
from ._lib import check_guidance_rescale, latent_shape
from .model import Session
from .utils import latent_mask, rescale


def encode_prompts(prompts, tokenizer, clip):
    """pipeline.mojo:39-54: ids = bpe_encode(prompt.replace(" ", "</w>")) -> CLIP.forward -> (B, 77, 768).
    Prompts longer than 77 ids are cut to 77 (the reference's `set_items` into a 77-wide row, clip.mojo:91-93)."""
    from .tokenizer import process_prompt
    if isinstance(prompts, str):
        prompts = [prompts]
    ids = np.zeros((len(prompts), 77), dtype=np.int32)
    for i, p in enumerate(prompts):
        t = tokenizer.bpe_encode(process_prompt(p))[:77]
        ids[i, : len(t)] = t
    return clip.forward(ids)


def generate(diffusion, decoder, context, uncond_context=None, strength=0.8, cfg=True, cfg_scale=7.5,
             inference_steps=50, seed_val=0, input_image=None, encoder=None, latents=None, noise=None,
             num_training_steps=1000, L=64, return_latents=False, sampler="ddpm", eta=0.0, spacing="leading", mask=None,
             mask_mode="any", seeds=None, guidance_rescale=0.0, prediction="epsilon", zero_terminal_snr=False, controlnet=None,
             control_image=None, control_scale=1.0, control_cond_only=False, control_start=0.0, control_end=1.0, ip_adapter=None,
             ip_image_embeds=None, ip_scale=1.0, ip_start=0.0, ip_end=1.0, ip_image=None, image_encoder=None, ip_hidden=None,
             ip_uncond_hidden=None, freeu=None):
    """context (B,T,768); returns images (B,3,8LH,8LW) in [0,255] like pipeline.mojo:127.  L is the latent side (64: 512x512) or a pair
    (LH, LW) for a rectangular image ((96, 64): 512 wide, 768 high); where the text below says L,L the tensor is LH,LW.

    sampler "ddpm" (the reference's, about 50 steps) | "ddim" (eta = 0: deterministic) | "dpmpp_2m" (second-order multistep, 20-25
    steps); spacing "leading" (the reference's timesteps) | "trailing" (starts at N - 1: few-step sampling).  The defaults are the
    reference's loop.  Noise is read by "ddpm" and by "ddim" with eta > 0.

    mask (B,1,8L,8L) or (B,8L,8L) in [0,1] with input_image and encoder: inpainting, 1 = regenerate, 0 = keep the image.  The loop is
    img2img's with the known region of the latents put back after every step (`Session.set_inpaint`), re-noised with the noise
    `add_noise` used; mask_mode "any" (a latent cell that touches a masked pixel is regenerated) | "area" (`latent_mask`).

    latents / noise default to N(0,1) from the counter RNG keyed by seed_val (App.A D19).

    seeds: a sequence of B ints, one per sample - the initial latents, the img2img / inpainting noise and every step's noise are drawn
    on the device from that sample's seed (`Session.set_seeds`), so a seed gives the same image wherever its sample sits in the batch
    and no noise tensor crosses the bus; only the encoder's noise input stays a host tensor keyed by seed_val.  Not with `noise` or
    `latents`.

    guidance_rescale in [0, 1] (Lin et al. 2023, eq. 15-16; diffusers' argument of the same name), with cfg=True: every step scales
    the guided prediction back towards the conditional prediction's per-sample standard deviation (`Session.set_guidance_rescale`);
    0.7 is the paper's value against the over-saturation of guidance scales of 7 and more.  0 is the reference's loop.

    prediction "epsilon" (the reference's models) | "v" (v-prediction models: SD-2.x-768-style checkpoints and v fine-tunes), and
    zero_terminal_snr=True for a model trained on the rescaled schedule of Lin et al. 2023 (algorithm 1), which wants "v" and
    spacing="trailing" so that sampling starts from pure noise (`Session.set_prediction`; `checkpoint.read_scheduler_config` maps a
    diffusers scheduler_config.json to these keywords).  The defaults are the reference's loop.

    controlnet, a `tsd.ControlNet` on the diffusion model's context (full-size UNet variants), with control_image (3,8LH,8LW) or
    (B,3,8LH,8LW), taken as given (diffusers feeds [0, 1]): every step whose index lies in [control_start, control_end] as fractions of
    the step list (diffusers' control_guidance_start / _end) runs the ControlNet and adds its residuals scaled by control_scale;
    control_cond_only: with cfg, only the conditional half is controlled (`Session.set_control`).

    ip_adapter, a `tsd.IPAdapter` on the diffusion model's context (full-size SD-1.x variants), with ip_image_embeds (1024,) or (B,1024),
    the CLIP image embedding of the prompt image (diffusers' ip_adapter_image_embeds) - or with the prompt image itself: ip_image
    (3,H,W) or (B,3,H,W) on the 0 .. 255 scale and image_encoder, a `tsd.CLIPVision` on the same context, whose `forward(ip_image)` gives
    those embeddings (`checkpoint.load_clip_vision` reads the `image_encoder/` folder the adapter files come with).
    Every step whose index lies in [ip_start, ip_end] as fractions of the step list adds the attention over the projected image tokens,
    scaled by ip_scale, in every cross-attention block.  With cfg the unconditional half reads the projection of a zero embedding, as
    diffusers does (`Session.set_ip_adapter`).

    A plus adapter (`tsd.IPAdapter(variant="ip_adapter_plus_sd15")`, `checkpoint.load_ip_adapter_plus`) reads the vision encoder's
    hidden states instead of the embedding: ip_image + image_encoder runs `image_encoder.forward(ip_image, hidden=True)` and
    `ip_adapter.resample` on the result; ip_hidden (S,1280) or (B,S,1280) is for callers who hold the hidden states (S = 257 from
    `CLIPVision`).  ip_image_embeds with a plus adapter and ip_hidden with a plain one are refused.  With cfg the unconditional half
    reads, as the published plus pipelines do, the resampled hidden states of the image that normalises to zero
    (`tsd.clip_neutral_image()`, a 224x224 constant the front end does not resample; its single fma leaves a few fp16 subnormals where
    the published code has exact zeros): computed here when image_encoder is given, or passed as ip_uncond_hidden, same shapes as
    ip_hidden.

    freeu, a dict of `Diffusion.set_freeu`'s keywords (dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2) are the paper's SD-1.x values): the
    model runs FreeU for this call, and holds the table it held before - or none - on every way out."""
    from .free_u import freeu_scope
    with freeu_scope(diffusion, freeu):
        return _generate(**{k: v for k, v in locals().items() if k not in ("freeu", "freeu_scope")})


def _generate(diffusion, decoder, context, uncond_context, strength, cfg, cfg_scale, inference_steps, seed_val, input_image, encoder, latents,
              noise, num_training_steps, L, return_latents, sampler, eta, spacing, mask, mask_mode, seeds, guidance_rescale, prediction,
              zero_terminal_snr, controlnet, control_image, control_scale, control_cond_only, control_start, control_end, ip_adapter,
              ip_image_embeds, ip_scale, ip_start, ip_end, ip_image, image_encoder, ip_hidden, ip_uncond_hidden):
    plus = bool(getattr(ip_adapter, "is_plus", False))
    if ip_hidden is not None and (ip_image is not None or ip_image_embeds is not None):
        raise ValueError("generate: pass one of ip_image, ip_image_embeds and ip_hidden, not both")
    if ip_image is not None and ip_image_embeds is not None:
        raise ValueError("generate: pass ip_image or ip_image_embeds, not both")
    if ip_uncond_hidden is not None and ip_hidden is None:
        raise ValueError("generate: ip_uncond_hidden goes with ip_hidden (with ip_image the unconditional hidden states are computed here)")
    if ip_hidden is not None:
        if ip_adapter is None:
            raise ValueError("generate: ip_hidden is the input of an IP-Adapter Plus: pass ip_adapter= as well")
        if not plus:
            raise ValueError("generate: ip_hidden is what a plus adapter reads (variant \"ip_adapter_plus_sd15\"); this ip_adapter reads "
                             "the 1024-wide image embedding: pass ip_image_embeds, or ip_image with image_encoder")
        if np.ndim(ip_hidden) not in (2, 3) or np.shape(ip_hidden)[-1] != 1280:
            raise ValueError(f"generate: ip_hidden must have shape (S, 1280) or (B, S, 1280), got {np.shape(ip_hidden)}")
        if cfg and ip_uncond_hidden is None and image_encoder is None:
            raise ValueError("generate: ip_hidden under cfg needs the unconditional half's hidden states: pass ip_uncond_hidden "
                             "(image_encoder.forward(tsd.clip_neutral_image(), hidden=True)[1]) or image_encoder")
    if plus and ip_image_embeds is not None:
        raise ValueError("generate: a plus adapter reads the vision encoder's hidden states, (S, 1280) per image, not the 1024-wide image "
                         "embedding: pass ip_hidden, or ip_image with image_encoder")
    if ip_image is not None and image_encoder is None:
        raise ValueError("generate: ip_image needs image_encoder (a tsd.CLIPVision) to turn the pixels into the image embedding")
    if (ip_adapter is None) != (ip_image_embeds is None and ip_image is None and ip_hidden is None):
        raise ValueError("generate: ip_adapter goes together with ip_image_embeds, ip_image or ip_hidden")
    if ip_image is not None:
        if np.ndim(ip_image) not in (3, 4) or np.shape(ip_image)[-3] != 3:
            raise ValueError(f"generate: ip_image must have shape (3, H, W) or (B, 3, H, W), got {np.shape(ip_image)}")
        if getattr(image_encoder.model, "ctx", None) is not diffusion.model.ctx:
            raise ValueError("generate: image_encoder and the diffusion model belong to different contexts")
    elif ip_hidden is not None and cfg and ip_uncond_hidden is None and getattr(image_encoder.model, "ctx", None) is not diffusion.model.ctx:
        raise ValueError("generate: image_encoder and the diffusion model belong to different contexts")
    if ip_adapter is not None and not (0.0 <= ip_start <= ip_end <= 1.0):
        raise ValueError(f"generate: ip_start / ip_end must satisfy 0 <= start <= end <= 1, got {ip_start}, {ip_end}")
    if (controlnet is None) != (control_image is None):
        raise ValueError("generate: controlnet and control_image go together")
    if controlnet is not None and not (0.0 <= control_start <= control_end <= 1.0):
        raise ValueError(f"generate: control_start / control_end must satisfy 0 <= start <= end <= 1, got {control_start}, {control_end}")
    guidance_rescale = check_guidance_rescale(guidance_rescale, cfg)
    if seeds is not None and (noise is not None or latents is not None):
        raise ValueError("generate(seeds=...) draws latents and noise on the device: pass neither noise nor latents")
    context = np.asarray(context, dtype=np.float32)
    if context.ndim == 2:
        context = context[None]
    B, T, _ = context.shape
    LH, LW = latent_shape(L)
    if mask is not None and (input_image is None or encoder is None):
        raise ValueError("generate(mask=...) needs input_image and encoder: the mask says which part of that image to keep")
    if not (0.0 <= strength <= 1.0):  # pipeline.mojo:23-29
        print("Strength must be between 0 and 1. Returning empty matrix")
        return np.zeros((0, 0, 0), dtype=np.float32)
    if mask is not None and np.shape(mask) not in ((B, 1, 8 * LH, 8 * LW), (B, 8 * LH, 8 * LW)):
        raise ValueError(f"mask must have shape {(B, 1, 8 * LH, 8 * LW)} or {(B, 8 * LH, 8 * LW)}, got {np.shape(mask)}")
    if input_image is not None and np.shape(input_image)[-2:] != (8 * LH, 8 * LW):
        raise ValueError(f"input_image must be {(8 * LH, 8 * LW)} pixels (rows, columns), got {np.shape(input_image)}")
    sess = Session(diffusion.model, decoder.model if decoder is not None else None, B, L, T, cfg=cfg)
    try:
        start = 0
        if input_image is not None:
            start = inference_steps - int(inference_steps * strength)  # sampler.mojo:68-70
        if (prediction, bool(zero_terminal_snr)) != ("epsilon", False):  # likewise: the default session never hears of it
            sess.set_prediction(prediction, zero_terminal_snr)
        if (sampler, eta, spacing) != ("ddpm", 0.0, "leading"):  # the default session is the reference's: nothing to set
            sess.set_sampler(sampler, eta, spacing)
        sess.set_schedule(num_training_steps, inference_steps, start)
        n = sess.num_steps
        nl = B * 4 * LH * LW
        if input_image is not None:  # pipeline.mojo:66-79
            img = rescale(input_image, (0, 255), (-1, 1))
            enc_noise = rng.normal(seed_val, 1, nl).reshape(B, 4, LH, LW)
            latents = encoder.forward(img, enc_noise)
            if mask is not None:
                mask_lat = latent_mask(mask, mask_mode, diffusion.model.ctx)
        elif latents is None:
            latents = np.zeros((B, 4, LH, LW), dtype=np.float32) if seeds is not None else rng.normal(seed_val, 2, nl).reshape(B, 4, LH, LW)
        if noise is None and seeds is None:
            noise = rng.normal(seed_val, 3, n * nl).reshape(n, B, 4, LH, LW)
        sess.upload(latents, context, uncond_context if cfg else None, noise, cfg_scale)
        if seeds is not None:
            sess.set_seeds(seeds)
            if input_image is None:
                sess.seed_latents()
            else:
                sess.add_noise_seeded(0)
                if mask is not None:
                    sess.set_inpaint(mask_lat, latents, seeded=True)
        elif input_image is not None:
            z4 = rng.normal(seed_val, 4, nl).reshape(B, 4, LH, LW)
            sess.add_noise(0, z4)  # sampler.mojo:111-124 at timesteps[0]
            if mask is not None:
                sess.set_inpaint(mask_lat, latents, z4)
        if guidance_rescale > 0.0:
            sess.set_guidance_rescale(guidance_rescale)
        if controlnet is not None:  # step i of n is controlled when control_start <= i / n and (i + 1) / n <= control_end, as diffusers keeps it
            first = int(np.ceil(control_start * n - 1e-9))
            last = int(np.floor(control_end * n + 1e-9)) - 1
            if last >= first:
                sess.set_control(controlnet, control_image, control_scale, control_cond_only, first, last)
        if ip_adapter is not None:
            first = int(np.ceil(ip_start * n - 1e-9))
            last = int(np.floor(ip_end * n + 1e-9)) - 1
            if last >= first and plus:
                def hidden_rows(h, what):
                    h = np.asarray(h, dtype=np.float32)
                    h = np.repeat(h[None], B, axis=0) if h.ndim == 2 else h
                    if h.ndim != 3 or h.shape[0] != B or h.shape[2] != 1280:
                        raise ValueError(f"generate: {what} must have shape (S, 1280) or ({B}, S, 1280), got {h.shape}")
                    return h
                h = hidden_rows(image_encoder.forward(ip_image, hidden=True)[1] if ip_image is not None else ip_hidden, "the hidden states")
                hu = None
                if cfg:  # the published pipelines' resample(hidden(encoder(zeros_like(normalised pixels))))
                    from .clip import clip_neutral_image
                    hu = hidden_rows(ip_uncond_hidden if ip_uncond_hidden is not None else image_encoder.forward(clip_neutral_image(), hidden=True)[1],
                                     "ip_uncond_hidden")
                sess.set_ip_adapter(ip_adapter, ip_adapter.resample(h), ip_adapter.resample(hu) if cfg else None, ip_scale, first, last)
            elif last >= first:
                e = np.asarray(image_encoder.forward(ip_image) if ip_image is not None else ip_image_embeds, dtype=np.float32)
                e = np.repeat(e[None], B, axis=0) if e.ndim == 1 else e
                if e.shape != (B, 1024):
                    raise ValueError(f"generate: the image embeddings must have shape (1024,) or ({B}, 1024), got {e.shape}")
                sess.set_ip_adapter(ip_adapter, ip_adapter.project(e), ip_adapter.project(np.zeros_like(e)) if cfg else None, ip_scale, first, last)
        for i in range(n):  # pipeline.mojo:87-122
            sess.step(i)
        out_lat = sess.latents()
        if decoder is None or return_latents:
            return out_lat
        sess.decode()
        return sess.images(rescale=True)
    finally:
        sess.close()   # on every way out: a refused argument or a failed step leaves no session behind
