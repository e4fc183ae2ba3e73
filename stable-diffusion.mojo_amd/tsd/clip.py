"""Host-side mirror of `clip.mojo`: CLIP text encoder (the step before the hot path).

`CLIP.forward(tokens)` is one call through the C ABI (`tsd_clip_forward`) with device-resident packed weights;
intended semantics only."""
import ctypes as C

import numpy as np

from ._lib import NULL_MATRIX, check, lib
from .model import Model


class CLIP:
    """`CLIP` clip.mojo:56-109: ClipEmbedding(49408, 768, 77) + 12 x ClipPlayer(12, 768) + LayerNorm(768).

    forward(tokens): int ids, shape (T,) or (B, T) with T <= 77 (zero-padded to 77 like clip.mojo:91-93)
    -> (77, 768) or (B, 77, 768) float32: the `context` of Diffusion.forward / generate."""

    def __init__(self, seed=0, ctx=None, params=None, variant="clip"):
        """variant "clip_torch" (extension): torch LayerNorms with weight / bias = Hugging Face's CLIPTextModel, for real
        checkpoints (tsd.checkpoint.load_clip_text).  variant "clip_sd2": the OpenCLIP-H text encoder as diffusers ships it for SD-2.x -
        width 1024, 16 heads, 23 layers, erf-GELU; forward gives (77, 1024) / (B, 77, 1024), ids past the prompt are 0."""
        self.model = Model(variant, ctx=ctx, seed=None if params is not None else seed)
        if params is not None:
            self.model.load_params(params)

    def forward(self, tokens):
        t = np.ascontiguousarray(np.asarray(tokens), dtype=np.int32)
        single = t.ndim == 1
        tb = t[None] if single else t
        B, T = tb.shape
        out = np.empty((B, 77, self.model.context_width), dtype=np.float32)
        code = lib().tsd_clip_forward(self.model.h, tb.ctypes.data_as(C.POINTER(C.c_int32)), B, T,
                                      out.ctypes.data_as(C.POINTER(C.c_float)))
        if check(code, True):
            return NULL_MATRIX()
        return out[0] if single else out


def _images(images, who):
    a = np.ascontiguousarray(images, dtype=np.float32)
    single = a.ndim == 3
    if single:
        a = a[None]
    if a.ndim != 4 or a.shape[1] != 3:
        raise ValueError(f"{who}: images must have shape (3, H, W) or (B, 3, H, W) on the 0 .. 255 scale, got {np.shape(images)}")
    return a, single


def clip_image_patches(images, ctx=None):
    """The vision encoder's image front end alone (`tsd_clip_image_patches_f16`): images (3,H,W) or (B,3,H,W) float on 0 .. 255, sides
    8 .. 2048 -> float16 (256, 592) or (B, 256, 592): resized (PIL's antialiased bicubic, shortest edge 224), centre-cropped to 224x224,
    normalised with CLIP's mean / std; row py * 16 + px, column c * 196 + kh * 14 + kw, columns 588 .. 591 zero."""
    from . import _lib
    a, single = _images(images, "clip_image_patches")
    B, _, H, W = a.shape
    out = np.empty((B, 256, 592), dtype=np.float16)
    check(lib().tsd_clip_image_patches_f16((ctx or _lib.default_context()).h, a.ctypes.data_as(C.POINTER(C.c_float)), B, H, W, out.ctypes.data))
    return out[0] if single else out


CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)


def clip_neutral_image():
    """The image the vision encoder's front end normalises to zero: (3, 224, 224) float32, channel c constant at 255 * mean_c.

    The published IP-Adapter Plus pipelines compute the unconditional image tokens from `zeros_like(normalised pixels)`; in this
    package's pixel convention (0 .. 255 in, normalisation inside the encoder) that input is this image.  At 224 x 224 the front end
    resamples nothing, and its single fma (v / (255 std_c) - mean_c / std_c on fp32 constants, rounded once to fp16) leaves a few fp16
    subnormals where the published code has exact zeros: the red channel comes out as -2 subnormal units (-1.2e-7), green and blue as
    zero; in exact arithmetic the image is within one unit (6e-8) of zero everywhere."""
    img = np.empty((3, 224, 224), dtype=np.float32)
    for c, m in enumerate(CLIP_IMAGE_MEAN):
        img[c] = np.float32(255.0 * m)
    return img


class CLIPVision:
    """The CLIP vision encoder the published `ip-adapter_sd15` files were trained against (no reference counterpart): OpenCLIP ViT-H/14 as
    Hugging Face ships it in the `image_encoder/` folder of h94/IP-Adapter - 14x14 patches of a 224x224 crop, 257 tokens of width 1280,
    32 pre-LN layers of 16 heads, erf-GELU MLP, post-LayerNorm of the class token, 1280 -> 1024 projection.

    forward(images): (3,H,W) or (B,3,H,W) float on the 0 .. 255 scale (what `generate(input_image=)` takes), sides 8 .. 2048, B <= 16
    -> (1024,) or (B,1024) float32, HF's `image_embeds`: the `ip_image_embeds` of `generate` / the input of `IPAdapter.project`.
    forward(images, hidden=True) -> (image_embeds, hidden) with hidden (257,1280) or (B,257,1280), HF's `hidden_states[-2]` (the input
    of the last layer, no post-LayerNorm).  The resize is the float form of CLIPImageProcessor's (`clip_image_patches`): it does not
    round the resized image to uint8; a 224x224 input is not resampled at all."""

    def __init__(self, seed=0, ctx=None, params=None, variant="clip_vision_h"):
        if variant != "clip_vision_h":
            raise ValueError(f"CLIPVision: unknown variant {variant!r} (clip_vision_h)")
        self.model = Model(variant, ctx=ctx, seed=None if params is not None else seed)
        if params is not None:
            self.model.load_params(params)

    def forward(self, images, hidden=False):
        a, single = _images(images, "CLIPVision.forward")
        B, _, H, W = a.shape
        fp = C.POINTER(C.c_float)
        emb = np.empty((B, 1024), dtype=np.float32)
        hid = np.empty((B, 257, 1280), dtype=np.float32) if hidden else None
        check(lib().tsd_clip_vision_forward(self.model.h, a.ctypes.data_as(fp), B, H, W, emb.ctypes.data_as(fp),
                                            hid.ctypes.data_as(fp) if hidden else None))
        if hidden:
            return (emb[0], hid[0]) if single else (emb, hid)
        return emb[0] if single else emb
