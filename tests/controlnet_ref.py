"""Numpy restatement of the ControlNet of the full-size UNet and of the controlled UNet forward, from oracle.models' block functions.

TEST INFRASTRUCTURE.  Single-sample functions in CHW, like oracle.models.  `controlnet` returns the 13 residuals (the twelve skips the
encoder pushes, in push order, then the bottleneck output, each through its zero convolution); `diffusion_sd15_controlled` is
oracle.models.diffusion_sd15 with s * r_i added to every popped skip and to the bottleneck output.  Parameters are drawn here in numpy
from the library's own inventory (names, shapes, bounds) and handed to both sides.
"""
import numpy as np

from oracle import models, ops
from oracle.models import _conv, time_embedding_mlp, unet_attention_block, unet_residual_block
from oracle.ops import DEFAULT
from oracle.spec import FULL_UNET_STEPS

ENC_N = 21  # steps of FULL_UNET_STEPS through the bottleneck: the first "pop" is step 22
HINT_STRIDES = (1, 1, 2, 1, 2, 1, 2, 1)
assert [f for _, _, f in FULL_UNET_STEPS[:ENC_N]].count("push") == 12 and FULL_UNET_STEPS[ENC_N][2] == "pop"
assert all(f != "pop" for _, _, f in FULL_UNET_STEPS[:ENC_N])


def draw_params(specs, seed, nonzero=()):
    """{name: fp32 array} for every used entry of `specs` ([(name, shape, used, bound)], tsd.param_specs): U(+-bound) from numpy's
    generator, norm weights 1 + U (their bound is 0.3).  A kernel whose name starts with one of `nonzero` and whose bound is 0 (a zero
    convolution, the hint encoder's last layer) gets 1 / sqrt(fan_in) instead: at zero every residual is zero."""
    g = np.random.default_rng(seed)
    out = {}
    for name, shape, used, bound in specs:
        if not used:
            continue
        if bound == 0.0 and name.endswith(".kernel") and name.startswith(tuple(nonzero)):
            bound = 1.0 / np.sqrt(float(np.prod(shape[1:])))
        if bound == 0.0:
            out[name] = np.zeros(shape, np.float32)
            continue
        a = g.uniform(-bound, bound, size=shape).astype(np.float32)
        is_norm_weight = name.endswith(".weight") and len(shape) == 1
        out[name] = a + np.float32(1.0) if is_norm_weight else a
    return out


def _layer(P, i, h, context, time, sem, tn):
    kind, a, _ = FULL_UNET_STEPS[i - 1]
    name = f"unet.layer{i}"
    if kind == "conv":
        return _conv(P, name, h, (1, 1), stride=(a[3], a[3]))
    if kind == "upconv":
        return _conv(P, name, ops.upsample_nearest2x(h), (1, 1))
    if kind == "res":
        return unet_residual_block(P, name, h, time, *a, tn=tn)
    return unet_attention_block(P, name, h, context, *a, sem=sem, tn=tn)


def hint_encoder(P, hint):
    """(3, 8LH, 8LW) -> (320, LH, LW): eight 3x3 convolutions, SiLU after each but the last."""
    h = hint
    for i, s in enumerate(HINT_STRIDES, start=1):
        h = _conv(P, f"hint.conv{i}", h, (1, 1), stride=(s, s))
        if i < len(HINT_STRIDES):
            h = ops.silu(h)
    return h


def controlnet(P, x, context, t320, hint, sem=DEFAULT, tn=False):
    """The 13 residuals of one sample: x (4,LH,LW), context (T,768), t320 (320,), hint (3,8LH,8LW)."""
    time = time_embedding_mlp(P, t320)
    feat = hint_encoder(P, hint)
    pushed = []
    h = x
    for i in range(1, ENC_N + 1):
        h = _layer(P, i, h, context, time, sem, tn)
        if i == 1:
            h = h + feat
        if FULL_UNET_STEPS[i - 1][2] == "push":
            pushed.append(h)
    res = [_conv(P, f"zero.skip{k + 1}", s, (0, 0)) for k, s in enumerate(pushed)]
    res.append(_conv(P, "zero.mid", h, (0, 0)))
    return res


def unet_full_controlled(P, x, context, time, res, s, sem=DEFAULT, tn=False):
    """oracle.models.unet_full with s * res[k] added to skip k when it is popped and s * res[12] to the bottleneck output."""
    skips = []
    h = x
    s = np.float32(s)
    for i, (_, _, flags) in enumerate(FULL_UNET_STEPS, start=1):
        if flags == "pop":
            k = len(skips) - 1
            h = ops.concat_channels(h, skips.pop() + s * res[k])
        h = _layer(P, i, h, context, time, sem, tn)
        if i == ENC_N:
            h = h + s * res[12]
        if flags == "push":
            skips.append(h)
    assert not skips
    return h


def diffusion_sd15_controlled(P, x, context, t320, res, s, sem=DEFAULT, tn=False):
    """oracle.models.diffusion_sd15 on the controlled graph; res = the 13 residuals (or None: uncontrolled)."""
    time = time_embedding_mlp(P, t320)
    if res is None:
        res, s = [np.float32(0.0)] * 13, 0.0
    h = unet_full_controlled(P, x, context, time, res, s, sem=sem, tn=tn)
    if tn:
        h = ops.silu(ops.group_norm_torch(h, 32, 1e-5, P["final.layer1.weight"], P["final.layer1.bias"]))
        return _conv(P, "final.layer2", h, (1, 1))
    return models.unet_output_layer(P, h)
