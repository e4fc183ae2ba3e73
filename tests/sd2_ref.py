"""Numpy restatement of the SD-2.x models (kinds "diffusion_sd2" and "clip_sd2") from the oracle's own block functions.

TEST INFRASTRUCTURE.  Single-sample functions in CHW, like oracle.models.  The UNet is oracle.spec.FULL_UNET_STEPS with every attention
block's (8, d_head) replaced by (C / 64, 64) - `unet_attention_block` takes n_head and n_embed - under torch norm semantics (tn: affine
norms, eps inside the root, erf-GELU in the GEGLU gate), on a 1024-wide context.  The text encoder is 23 `clip_layer`s restated with
torch's exact GELU in place of quick-GELU (`ops.gelu_erf`, `ops.self_attention` with 16 heads), width 1024, and the final LayerNorm.
Parameters are drawn in numpy from the library's own inventory (tsd.param_specs(kind): names, shapes, bounds) with a seed, as
tests/controlnet_ref.py does, and handed to both sides.
"""
import numpy as np

from controlnet_ref import draw_params  # noqa: F401  (re-exported: the one way tests draw parameters from an inventory)
from oracle import ops
from oracle.models import _conv, _lin, _ln, time_embedding_mlp, unet_attention_block, unet_residual_block
from oracle.ops import DEFAULT
from oracle.spec import FULL_UNET_STEPS

CTX_WIDTH = 1024
HEAD_DIM = 64
CLIP_LAYERS, CLIP_HEADS, CLIP_WIDTH = 23, 16, 1024


def sd2_steps():
    """FULL_UNET_STEPS with head dimension 64 in every attention block."""
    out = []
    for kind, a, flags in FULL_UNET_STEPS:
        if kind == "attn":
            C = a[0] * a[1]
            assert C % HEAD_DIM == 0
            a = (C // HEAD_DIM, HEAD_DIM)
        out.append((kind, a, flags))
    return out


SD2_STEPS = sd2_steps()
assert [a for k, a, _ in SD2_STEPS if k == "attn"][:7:2] == [(5, 64), (10, 64), (20, 64), (20, 64)]


def unet_sd2(P, x, context, time, sem=DEFAULT):
    skips = []
    h = x
    for i, (kind, a, flags) in enumerate(SD2_STEPS, start=1):
        name = f"unet.layer{i}"
        if flags == "pop":
            h = ops.concat_channels(h, skips.pop())
        if kind == "conv":
            h = _conv(P, name, h, (1, 1), stride=(a[3], a[3]))
        elif kind == "upconv":
            h = _conv(P, name, ops.upsample_nearest2x(h), (1, 1))
        elif kind == "res":
            h = unet_residual_block(P, name, h, time, *a, tn=True)
        else:
            h = unet_attention_block(P, name, h, context, *a, sem=sem, tn=True)
        if flags == "push":
            skips.append(h)
    assert not skips
    return h


def diffusion_sd2(P, x, context, t320, sem=DEFAULT):
    """x (4,LH,LW), context (T,1024), t320 (320,) -> (4,LH,LW)."""
    assert context.shape[-1] == CTX_WIDTH
    time = time_embedding_mlp(P, t320)
    h = unet_sd2(P, x, context, time, sem=sem)
    h = ops.silu(ops.group_norm_torch(h, 32, 1e-5, P["final.layer1.weight"], P["final.layer1.bias"]))
    return _conv(P, "final.layer2", h, (1, 1))


def clip_sd2_layer(P, prefix, x, sem=DEFAULT):
    res = x
    h = _ln(P, prefix + ".layer1", x, sem, True)
    h = ops.self_attention(h, CLIP_HEADS, P[prefix + ".layer2.in_proj.weight"], P[prefix + ".layer2.in_proj.bias"],
                           P[prefix + ".layer2.out_proj.weight"], P[prefix + ".layer2.out_proj.bias"], causal=True, sem=sem)
    x = h + res
    res = x
    h = _ln(P, prefix + ".layer3", x, sem, True)
    h = ops.gelu_erf(_lin(P, prefix + ".layer4", h))
    return _lin(P, prefix + ".layer5", h) + res


def clip_sd2(P, tokens, sem=DEFAULT, n_token=77):
    """token ids (<= 77; the ids past the prompt are 0) -> (77, 1024)."""
    t = np.zeros(n_token, dtype=np.int64)
    tokens = np.asarray(tokens, dtype=np.int64).reshape(-1)
    t[: len(tokens)] = tokens
    x = ops.embedding(t, P["embedding.token.weight"]) + P["embedding.position"].reshape(n_token, -1)
    for i in range(1, CLIP_LAYERS + 1):
        x = clip_sd2_layer(P, f"player{i}", x, sem=sem)
    return _ln(P, "layernorm", x, sem, True)
