"""tsd - Python host side of libtsd.so, mirroring the reference's Mojo modules for the hot path.

  tsd.utils      <-> helpers/utils.mojo     Conv2D, GroupNorm, SiLU, Gelu, Linear, Upsample, LayerNorm, Softmax, ...
  tsd.attention  <-> helpers/attention.mojo Self_Attention, Cross_Attention
  tsd.diffusion  <-> diffusion.mojo         Time_Embedding, Unet_Residual_Block, Unet_Attention_Block, UNet, Diffusion
                 (+ ControlNet, which has no reference counterpart: spatial conditioning of the full-size UNet, Diffusion.forward(control=...);
                  and IPAdapter: image-prompt tokens through decoupled cross attention, Diffusion.forward(ip_adapter=...))
  tsd.vae        <-> vae.mojo               Attention_Block, Res_Block, Decoder, Encoder
  tsd.sampler    <-> sampler.mojo           DDPMSampler (+ DDIMSampler, DPMSolverMultistepSampler: no reference counterpart)
  tsd.clip       <-> clip.mojo              CLIP text encoder (token ids -> context)
                 (+ CLIPVision, which has no reference counterpart: pixels -> the image embedding an IPAdapter projects)
  tsd.tokenizer  <-> helpers/utils.mojo     Tokenizer, bpe_encode (host-only logic inside libtsd)
  tsd.pipeline   <-> pipeline.mojo          generate (hot loop; the context embedding is an input)
  tsd.serve      (no reference counterpart) continuous batching over a slot session: SlotScheduler, generate_stream
  tsd.free_u     (no reference counterpart) FreeU on the full-size UNets: freeu_table, Diffusion.set_freeu, generate(freeu=...)
  tsd.lora       (no reference counterpart) LoRA adapters merged into the packed weights on the device, removable exactly
  tsd.ext        (no reference counterpart) torch-style GroupNorm / LayerNorm for real checkpoints

Every forward() is a call through the C ABI in include/tsd.h into hand-written HIP kernels for gfx950.
There is no CPU fallback.
"""
from . import _lib, rng  # noqa: F401
from . import ext  # noqa: F401  (non-reference extensions: torch-style norms)
from ._lib import Context, TsdError, default_context, device_ledger, set_default_context, set_strict  # noqa: F401
from .model import Model, Session, flop_count, param_specs  # noqa: F401
from .utils import (Conv2D, Gelu, GroupNorm, LayerNorm, Linear, SiLU, Softmax, Upsample, alphas_cumprod, cfg_rescale, concat,  # noqa: F401
                    control_inject, ddpm_step, get_time_embedding, inpaint_blend, ip_attn_add, latent_mask, matmul, normal_fill, pad, rescale, sampler_step_v)
from .attention import Cross_Attention, Self_Attention  # noqa: F401
from .diffusion import (ControlNet, Diffusion, IPAdapter, Time_Embedding, UNet, UNet_Output_Layer, Unet_Attention_Block,  # noqa: F401
                        Unet_Residual_Block)
from .vae import Attention_Block, Decoder, Encoder, Res_Block  # noqa: F401
from .clip import CLIP, CLIPVision, clip_image_patches, clip_neutral_image  # noqa: F401
from .tokenizer import Tokenizer, process_prompt  # noqa: F401
from .sampler import DDIMSampler, DDPMSampler, DPMSolverMultistepSampler  # noqa: F401
from .pipeline import encode_prompts, generate  # noqa: F401
from .serve import Request, SlotScheduler, generate_stream  # noqa: F401
from .free_u import freeu, freeu_table  # noqa: F401
from .lora import load_lora, lora_targets, merge_reference, read_lora  # noqa: F401
