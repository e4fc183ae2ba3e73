"""Host-side mirror of `diffusion.mojo`: same struct names, constructor arguments and forward() meaning.

`Diffusion` is the measured module (device-resident weights, one C call per forward).  The block
structs (`Time_Embedding`, `Unet_Residual_Block`, `Unet_Attention_Block`, `UNet_Output_Layer`) are
one C call per block with host weights, and `UNet` composes them exactly like diffusion.mojo:228-273 -
the per-struct drop-in surface.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NULL_MATRIX, check, f32, fp, lib, ptr
from .attention import Cross_Attention, Self_Attention
from .model import Model
from .utils import Conv2D, GroupNorm, LayerNorm, Linear, SiLU, Upsample, _ctx, concat


class Time_Embedding:
    """`Time_Embedding` diffusion.mojo:5-21."""

    def __init__(self, n_embed, seed=0, ctx=None):
        self.ctx = ctx
        self.layer1 = Linear(n_embed, 4 * n_embed, seed=seed, ctx=ctx)
        self.layer2 = Linear(4 * n_embed, 4 * n_embed, seed=seed, ctx=ctx)

    def forward(self, x):
        t = f32(x).reshape(-1)
        if t.size != 320 or self.layer1.out_features != 1280:
            print("Invalid input dimensions for Time_Embedding. Returning null matrix")
            return NULL_MATRIX()
        y = np.empty(1280, dtype=np.float32)
        check(lib().tsd_time_embedding_mlp_f32(_ctx(self.ctx), ptr(t), ptr(f32(self.layer1.weight)), ptr(f32(self.layer1.bias)),
                                               ptr(f32(self.layer2.weight)), ptr(f32(self.layer2.bias)), ptr(y)))
        return y.reshape(1, 1, 1280)


class Unet_Residual_Block:
    """`Unet_Residual_Block` diffusion.mojo:24-72."""

    def __init__(self, in_channels, out_channels, n_time=1280, seed=0, ctx=None):
        self.in_channels, self.out_channels, self.ctx = in_channels, out_channels, ctx
        self.layer1 = GroupNorm(32, in_channels)
        self.layer2 = Conv2D(in_channels, out_channels, 3, (1, 1), seed=seed)
        self.layer3 = Linear(n_time, out_channels, seed=seed)
        self.layer4 = GroupNorm(32, out_channels)
        self.layer5 = Conv2D(out_channels, out_channels, 3, (1, 1), seed=seed)
        self.layer6 = Conv2D(in_channels, out_channels, 1, (0, 0), seed=seed)

    def forward(self, x, time):
        x = f32(x)
        Cx, H, W = x.shape
        y = np.empty((self.out_channels, H, W), dtype=np.float32)
        t = f32(time).reshape(-1)
        code = lib().tsd_unet_residual_block_f32(
            _ctx(self.ctx), ptr(x), Cx, H, W, ptr(t), self.in_channels, self.out_channels,
            ptr(f32(self.layer2.kernel)), ptr(f32(self.layer2.bias)), ptr(f32(self.layer3.weight)), ptr(f32(self.layer3.bias)),
            ptr(f32(self.layer5.kernel)), ptr(f32(self.layer5.bias)), ptr(f32(self.layer6.kernel)), ptr(f32(self.layer6.bias)),
            ptr(y))
        return NULL_MATRIX() if check(code, True) else y


class Unet_Attention_Block:
    """`Unet_Attention_Block` diffusion.mojo:75-147."""

    def __init__(self, n_head, n_embed, d_context=768, seed=0, ctx=None):
        channels = n_head * n_embed
        self.n_head, self.n_embed, self.ctx = n_head, n_embed, ctx
        self.layer1 = GroupNorm(32, channels, epsilon=1e-6)
        self.layer2 = Conv2D(channels, channels, 1, (0, 0), seed=seed)
        self.layer3 = LayerNorm(channels)
        self.layer4 = Self_Attention(n_head, channels, in_bias=False, seed=seed)
        self.layer5 = LayerNorm(channels)
        self.layer6 = Cross_Attention(n_head, channels, d_context, in_bias=False, seed=seed)
        self.layer7 = LayerNorm(channels)
        self.layer8 = Linear(channels, 8 * channels, seed=seed)
        self.layer9 = Linear(4 * channels, channels, seed=seed)
        self.layer10 = Conv2D(channels, channels, 1, (0, 0), seed=seed)

    def weight_list(self):
        l4, l6 = self.layer4, self.layer6
        return [self.layer2.kernel, self.layer2.bias, l4.in_proj.weight, l4.out_proj.weight, l4.out_proj.bias,
                l6.q_proj.weight, l6.k_proj.weight, l6.v_proj.weight, l6.out_proj.weight, l6.out_proj.bias,
                self.layer8.weight, self.layer8.bias, self.layer9.weight, self.layer9.bias,
                self.layer10.kernel, self.layer10.bias]

    def forward(self, x, context):
        x = f32(x)
        Cx, H, W = x.shape
        c = f32(context)
        c = c[0] if c.ndim == 3 else c
        ws = [f32(w) for w in self.weight_list()]
        arr = (fp * len(ws))(*[ptr(w) for w in ws])
        y = np.empty_like(x)
        code = lib().tsd_unet_attention_block_f32(_ctx(self.ctx), ptr(x), self.n_head, self.n_embed, H, W, ptr(c),
                                                  c.shape[0], c.shape[1], arr, len(ws), ptr(y))
        return NULL_MATRIX() if check(code, True) else y


class UNet:
    """`UNet` diffusion.mojo:150-273 composed from the block structs (per-struct drop-in path)."""

    def __init__(self, seed=0, ctx=None):
        R, A = Unet_Residual_Block, Unet_Attention_Block
        k = dict(seed=seed, ctx=ctx)
        self.layer1 = Conv2D(4, 320, 3, (1, 1), **k)
        self.layer2, self.layer3 = R(320, 320, **k), A(8, 40, **k)
        self.layer4 = Conv2D(320, 320, 3, (1, 1), (2, 2), **k)
        self.layer5, self.layer6 = R(320, 640, **k), A(8, 80, **k)
        self.layer7 = Conv2D(640, 640, 3, (1, 1), (2, 2), **k)
        self.layer8, self.layer9 = R(640, 1280, **k), A(8, 160, **k)
        self.layer10, self.layer11 = R(2560, 1280, **k), A(8, 160, **k)
        self.layer12, self.layer13 = R(1920, 1280, **k), A(8, 160, **k)
        self.layer14 = Upsample(1280, ctx=ctx)
        self.layer15, self.layer16 = R(1280, 640, **k), A(8, 80, **k)
        self.layer17, self.layer18 = R(960, 640, **k), A(8, 80, **k)
        self.layer19 = Upsample(640, ctx=ctx)
        self.layer20, self.layer21 = R(640, 320, **k), A(8, 40, **k)
        self.layer22, self.layer23 = R(640, 320, **k), A(8, 40, **k)

    def forward(self, x, context, time):
        out = self.layer1.forward(x); skip1 = out
        out = self.layer2.forward(out, time); out = self.layer3.forward(out, context); skip2 = out
        out = self.layer4.forward(out); skip3 = out
        out = self.layer5.forward(out, time); out = self.layer6.forward(out, context); skip4 = out
        out = self.layer7.forward(out); skip5 = out
        out = self.layer8.forward(out, time); out = self.layer9.forward(out, context); skip6 = out
        out = concat(out, skip6, 0); out = self.layer10.forward(out, time); out = self.layer11.forward(out, context)
        out = concat(out, skip5, 0); out = self.layer12.forward(out, time); out = self.layer13.forward(out, context)
        out = self.layer14.forward(out)
        out = concat(out, skip4, 0); out = self.layer15.forward(out, time); out = self.layer16.forward(out, context)
        out = concat(out, skip3, 0); out = self.layer17.forward(out, time); out = self.layer18.forward(out, context)
        out = self.layer19.forward(out)
        out = concat(out, skip2, 0); out = self.layer20.forward(out, time); out = self.layer21.forward(out, context)
        out = concat(out, skip1, 0); out = self.layer22.forward(out, time); out = self.layer23.forward(out, context)
        return out


class UNet_Output_Layer:
    """`UNet_Output_Layer` diffusion.mojo:275-291 (composed: GroupNorm(320 groups) -> SiLU -> Conv2D)."""

    def __init__(self, in_channels, out_channels, seed=0, ctx=None):
        self.layer1 = GroupNorm(320, in_channels, ctx=ctx)
        self.layer2 = Conv2D(in_channels, out_channels, 3, (1, 1), seed=seed, ctx=ctx)
        self.ctx = ctx

    def forward(self, x):
        out = self.layer1.forward(x)
        out = SiLU(self.ctx).forward(out)
        return self.layer2.forward(out)


class Diffusion:
    """`Diffusion` diffusion.mojo:294-318 - device-resident weights; forward is ONE libtsd call.

    forward(x, context, time): x (4,LH,LW) or (B,4,LH,LW), square or not; context (T,768)/(1,T,768) or (B,T,768);
    time = get_time_embedding(t): (1,1,320) or (B,320)."""

    def __init__(self, seed=0, ctx=None, params=None, variant="diffusion"):
        """variant: "diffusion" (the reference's 23-layer Tiny-SD graph) or "diffusion_sd15" (full-size 860 M UNet,
        BASELINE configs[4]; same blocks, not defined by the reference) or "diffusion_sd15_torch" (that graph with the
        norm semantics and parameters of PyTorch-trained SD-1.x checkpoints, see tsd.checkpoint) or "diffusion_sd2" (the SD-2.x UNet:
        that graph with head dimension 64 in every attention block and a 1024-wide context, tsd.checkpoint.load_sd2_unet)."""
        self.model = Model(variant, ctx=ctx, seed=None if params is not None else seed)
        if params is not None:
            self.model.load_params(params)

    def forward(self, x, context, time, control=None, hint=None, control_scale=1.0, ip_adapter=None, ip_tokens=None, ip_scale=1.0):
        """control: a `ControlNet` on the same context, with hint (3,8LH,8LW) or (B,3,8LH,8LW) and control_scale a scalar or one value per
        sample - the ControlNet's residuals, scaled per sample, are added to the skips and the bottleneck output (full-size variants).
        ip_adapter: an `IPAdapter` on the same context, with ip_tokens (N,768) or (B,N,768), 1 <= N <= 16 (`IPAdapter.project`, or tokens
        from outside), and ip_scale a scalar or one value per sample - every cross-attention block adds the attention over the image
        tokens, scaled per sample, to the text result (full-size SD-1.x variants; `tsd_diffusion_forward_ip_hw`).  Both compose."""
        xb, c, t, single = _forward_inputs(x, context, time)
        B, _, LH, LW = xb.shape
        W = self.model.context_width
        if c.ndim != 3 or c.shape[0] != B or c.shape[2] != W:
            raise ValueError(f"context must have shape (T, {W}) or ({B}, T, {W}), got {np.shape(context)}: this UNet reads a {W}-wide context")
        out = np.empty_like(xb)
        if ip_adapter is None and ip_tokens is not None:
            raise ValueError("ip_tokens are the IP-Adapter's input: pass ip_adapter= as well")
        if ip_adapter is not None:
            tok = _ip_tokens_input(ip_tokens, B)
            si = np.ascontiguousarray(np.broadcast_to(np.asarray(ip_scale, dtype=np.float32), (B,)))
            if control is None and hint is not None:
                raise ValueError("hint is the ControlNet's input: pass control= as well")
            h = _hint_input(hint, B, LH, LW) if control is not None else None
            s = np.ascontiguousarray(np.broadcast_to(np.asarray(control_scale, dtype=np.float32), (B,))) if control is not None else None
            code = lib().tsd_diffusion_forward_ip_hw(self.model.h, ip_adapter.model.h, ptr(tok), tok.shape[1], ptr(si),
                                                     control.model.h if control is not None else None, ptr(h) if h is not None else None,
                                                     ptr(s) if s is not None else None, ptr(xb), ptr(c), ptr(t), B, LH, LW, c.shape[1], ptr(out))
        elif control is None:
            if hint is not None:
                raise ValueError("hint is the ControlNet's input: pass control= as well")
            code = lib().tsd_diffusion_forward_hw(self.model.h, ptr(xb), ptr(c), ptr(t), B, LH, LW, c.shape[1], ptr(out))
        else:
            h = _hint_input(hint, B, LH, LW)
            s = np.ascontiguousarray(np.broadcast_to(np.asarray(control_scale, dtype=np.float32), (B,)))
            code = lib().tsd_diffusion_forward_control_hw(self.model.h, control.model.h, ptr(xb), ptr(c), ptr(t), ptr(h), ptr(s), B, LH, LW,
                                                          c.shape[1], ptr(out))
        if check(code, True):
            return NULL_MATRIX()
        return out[0] if single else out

    def set_freeu(self, b1=None, b2=None, s1=None, s2=None, convention="diffusers", modulated=False, table=None):
        """FreeU (Si et al. 2023; diffusers' `enable_freeu(s1, s2, b1, b2)`) on a full-size variant: from the next forward on - a step of an
        open `Session` included - every decoder concat scales the backbone half of its hidden input by b and the four lowest spatial
        frequencies of its skip by s (`tsd_model_set_freeu`).  b1 / b2 / s1 / s2 fill the 12-entry table by `convention`
        (`tsd.freeu_table`: "diffusers" | "channels"), or table=(b[12], s[12]) gives it directly; modulated=True is the "v2" form of the
        authors' repository (b modulated per pixel by the min-max normalised channel mean).  A table of all ones is off."""
        from .free_u import freeu_arguments
        b, s, mode = freeu_arguments(b1, b2, s1, s2, convention, modulated, table)
        check(lib().tsd_model_set_freeu(self.model.h, ptr(b), ptr(s), mode))

    def clear_freeu(self):
        check(lib().tsd_model_set_freeu(self.model.h, None, None, 0))

    @property
    def freeu(self):
        """None when FreeU is off, else (b[12], s[12], mode) as the model holds them (`tsd_model_freeu`)."""
        b, s, mode = np.empty(12, np.float32), np.empty(12, np.float32), C.c_int(0)
        on = lib().tsd_model_freeu(self.model.h, ptr(b), ptr(s), C.byref(mode))
        if on < 0:
            check(on)
        return (b, s, mode.value) if on else None


def _ip_tokens_input(tokens, B):
    """Image tokens as a contiguous fp32 (B, N, 768) array, 1 <= N <= 16; (N, 768) is repeated for every sample."""
    if tokens is None:
        raise ValueError("an IP-Adapter needs its image tokens (IPAdapter.project(image_embeds))")
    t = f32(tokens)
    if t.ndim == 2:
        t = t[None]
    if t.ndim == 3 and t.shape[0] == 1 and B > 1:
        t = np.repeat(t, B, axis=0)
    if t.ndim != 3 or t.shape[0] != B or not (1 <= t.shape[1] <= 16) or t.shape[2] != 768:
        raise ValueError(f"ip_tokens must have shape (N, 768) or ({B}, N, 768) with 1 <= N <= 16, got {np.shape(tokens)}")
    return f32(t)


class IPAdapter:
    """IP-Adapter of the full-size SD-1.x UNet (Ye et al. 2023; the layout of the published ip-adapter_sd15 files) - device-resident
    weights: the image projection and one to_k_ip / to_v_ip pair per cross-attention block (model kind "ip_adapter_sd15").
    project(image_embeds) -> the N = 4 image tokens; `Diffusion.forward(ip_adapter=, ip_tokens=, ip_scale=)`, `Session.set_ip_adapter`
    and `generate(ip_adapter=, ip_image_embeds=)` consume them.  The 1024-wide image embedding (diffusers' `ip_adapter_image_embeds`)
    comes from the CLIP vision encoder, `tsd.CLIPVision.forward(image)`, or from the caller; `generate(ip_adapter=, ip_image=,
    image_encoder=)` runs the encoder itself.  See tsd.checkpoint.load_ip_adapter / load_clip_vision.

    variant "ip_adapter_plus_sd15": the layout of the published ip-adapter-plus_sd15 / ip-adapter-plus-face_sd15 files - the same 16
    pairs behind a Perceiver resampler (4 layers, 16 learned queries, 12 heads of 64) in place of the linear projection.
    resample(hidden) -> the N = 16 image tokens from the vision encoder's hidden states, `CLIPVision.forward(image, hidden=True)[1]`;
    everything that consumes tokens takes them unchanged, and `generate(ip_adapter=, ip_image=, image_encoder=)` or
    `generate(ip_adapter=, ip_hidden=)` runs the resampler itself.  See tsd.checkpoint.load_ip_adapter_plus."""
    N_TOKENS = 4
    VARIANTS = {"ip_adapter_sd15": 4, "ip_adapter_plus_sd15": 16}

    def __init__(self, seed=0, ctx=None, params=None, variant="ip_adapter_sd15"):
        if variant not in self.VARIANTS:
            raise ValueError(f"IPAdapter: unknown variant {variant!r} ({', '.join(self.VARIANTS)})")
        self.variant = variant
        self.n_tokens = self.VARIANTS[variant]
        self.model = Model(variant, ctx=ctx, seed=None if params is not None else seed)
        if params is not None:
            self.model.load_params(params)

    @property
    def is_plus(self):
        return self.variant == "ip_adapter_plus_sd15"

    def project(self, image_embeds):
        """(1024,) or (B, 1024) image embeddings -> tokens (4, 768) / (B, 4, 768) = LayerNorm(Linear(e)) (`tsd_ip_adapter_project`).
        A plus adapter has no such projection: TsdError with the library's message, which names `resample`'s entry."""
        e = f32(image_embeds)
        single = e.ndim == 1
        eb = f32(e[None] if single else e)
        if eb.ndim != 2 or eb.shape[1] != 1024:
            raise ValueError(f"image_embeds must have shape (1024,) or (B, 1024), got {e.shape}")
        out = np.empty((eb.shape[0], self.n_tokens, 768), dtype=np.float32)
        if check(lib().tsd_ip_adapter_project(self.model.h, ptr(eb), eb.shape[0], ptr(out)), True):
            return NULL_MATRIX()
        return out[0] if single else out

    def resample(self, hidden):
        """Plus adapters: (S, 1280) or (B, S, 1280) hidden states of the CLIP vision encoder (its `hidden_states[-2]`: S = 257; any
        1 <= S <= 1024), B <= 16 -> tokens (16, 768) / (B, 16, 768), the Perceiver resampler (`tsd_ip_adapter_resample`); every value is
        exactly an fp16.  An adapter of the plain kind has no resampler: TsdError with the library's message."""
        h = f32(hidden)
        single = h.ndim == 2
        hb = f32(h[None] if single else h)
        if hb.ndim != 3 or hb.shape[2] != 1280:
            raise ValueError(f"hidden must have shape (S, 1280) or (B, S, 1280), got {h.shape}")
        out = np.empty((hb.shape[0], 16, 768), dtype=np.float32)
        if check(lib().tsd_ip_adapter_resample(self.model.h, ptr(hb), hb.shape[0], hb.shape[1], ptr(out)), True):
            return NULL_MATRIX()
        return out[0] if single else out


def _forward_inputs(x, context, time):
    """The inputs of `Diffusion.forward` / `ControlNet.forward` as batched contiguous fp32 arrays: (latents, context, time, single)."""
    x = f32(x)
    single = x.ndim == 3
    xb = x[None] if single else x
    if xb.ndim != 4 or xb.shape[1] != 4:
        raise ValueError(f"latents must have shape (4, LH, LW) or (B, 4, LH, LW), got {x.shape}")
    B = xb.shape[0]
    c = f32(context)
    if c.ndim == 2:
        c = c[None]
    if c.shape[0] == 1 and B > 1:
        c = np.repeat(c, B, axis=0)
    t = f32(time).reshape(-1, 320)
    if t.shape[0] == 1 and B > 1:
        t = np.repeat(t, B, axis=0)
    return f32(xb), f32(c), f32(t), single


def _hint_input(hint, B, LH, LW):
    if hint is None:
        raise ValueError("a ControlNet needs its hint image")
    h = f32(hint)
    if h.ndim == 3:
        h = h[None]
    if h.shape[0] == 1 and B > 1:
        h = np.repeat(h, B, axis=0)
    if h.shape != (B, 3, 8 * LH, 8 * LW):
        raise ValueError(f"the hint must have shape (3, {8 * LH}, {8 * LW}) or ({B}, 3, {8 * LH}, {8 * LW}), got {np.shape(hint)}")
    return f32(h)


# (C, divisor of the latent side) of the 13 residuals: the twelve skips in push order, then the bottleneck output
CONTROL_RESIDUAL_SHAPES = ((320, 1), (320, 1), (320, 1), (320, 2), (640, 2), (640, 2), (640, 4), (1280, 4), (1280, 4), (1280, 8), (1280, 8),
                           (1280, 8), (1280, 8))


class ControlNet:
    """ControlNet of the full-size UNet (Zhang et al. 2023; the layout of diffusers' `ControlNetModel`) - device-resident weights.

    variant: "controlnet_sd15" (the reference's norms, pairs with "diffusion_sd15") or "controlnet_sd15_torch" (the norm semantics and
    parameters of PyTorch-trained checkpoints, pairs with "diffusion_sd15_torch"; see tsd.checkpoint.load_controlnet).  A seeded init
    leaves the zero convolutions at zero, as an untrained ControlNet has them: its residuals are all zero.
    forward(x, context, time, hint) -> the 13 residuals [(B,C_i,H_i,W_i)] (CONTROL_RESIDUAL_SHAPES); `Diffusion.forward(control=...)` runs both models
    in one call and is the consumer."""

    def __init__(self, seed=0, ctx=None, params=None, variant="controlnet_sd15"):
        if variant not in ("controlnet_sd15", "controlnet_sd15_torch"):
            raise ValueError(f"unknown ControlNet variant {variant!r}")
        self.model = Model(variant, ctx=ctx, seed=None if params is not None else seed)
        if params is not None:
            self.model.load_params(params)

    def hint(self, hint):
        """The hint encoder alone (`tsd_controlnet_hint_hw`): (3,8LH,8LW) or (B,3,8LH,8LW) -> features (320,LH,LW) / (B,320,LH,LW).
        It depends on the hint only: a denoise session runs it once."""
        h = f32(hint)
        single = h.ndim == 3
        hb = f32(h[None] if single else h)
        if hb.ndim != 4 or hb.shape[1] != 3 or hb.shape[2] % 8 or hb.shape[3] % 8:
            raise ValueError(f"the hint must have shape (3, 8LH, 8LW) or (B, 3, 8LH, 8LW), got {h.shape}")
        B, _, H, W = hb.shape
        out = np.empty((B, 320, H // 8, W // 8), dtype=np.float32)
        if check(lib().tsd_controlnet_hint_hw(self.model.h, ptr(hb), B, H // 8, W // 8, ptr(out)), True):
            return NULL_MATRIX()
        return out[0] if single else out

    def forward(self, x, context, time, hint):
        xb, c, t, single = _forward_inputs(x, context, time)
        B, _, LH, LW = xb.shape
        h = _hint_input(hint, B, LH, LW)
        outs = [np.empty((B, ch, LH // d, LW // d), dtype=np.float32) for ch, d in CONTROL_RESIDUAL_SHAPES]
        arr = (fp * len(outs))(*[ptr(o) for o in outs])
        code = lib().tsd_controlnet_forward_hw(self.model.h, ptr(xb), ptr(c), ptr(t), ptr(h), B, LH, LW, c.shape[1], arr)
        if check(code, True):
            return NULL_MATRIX()
        return [o[0] for o in outs] if single else outs
