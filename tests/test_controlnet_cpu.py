"""CPU: the ControlNet kinds' parameter inventory, the diffusers ControlNetModel key map, the numpy reference's own consistency and the
exported symbols.  No GPU: the inventory and the key map are host code, the reference is numpy."""
import numpy as np
import pytest

import controlnet_ref as R
from oracle import models, ops, rng
from oracle import spec as S

HINT = ((3, 16), (16, 16), (16, 32), (32, 32), (32, 96), (96, 96), (96, 256), (256, 320))
ZERO_WIDTHS = (320,) * 4 + (640,) * 3 + (1280,) * 5
NEW_SYMBOLS = ("tsd_controlnet_forward_hw", "tsd_diffusion_forward_control_hw", "tsd_control_inject_f16", "tsd_debug_set_control_stats",
               "tsd_controlnet_hint_hw", "tsd_session_set_control", "tsd_session_control_active")


def _expected(torch):
    """The inventory restated from oracle.spec's builders: time embedding, hint encoder, the UNet's steps through the bottleneck, the zero
    convolutions; the torch kind's norm parameters last."""
    out = []
    S._lin(out, "time_embed.layer1", 320, 1280)
    S._lin(out, "time_embed.layer2", 1280, 1280)
    for i, (cin, cout) in enumerate(HINT, start=1):
        S._conv(out, f"hint.conv{i}", cin, cout, 3)
    steps = S.FULL_UNET_STEPS[:R.ENC_N]
    for i, (kind, a, _) in enumerate(steps, start=1):
        name = f"unet.layer{i}"
        if kind == "conv":
            S._conv(out, name, a[0], a[1], a[2])
        elif kind == "res":
            S._unet_res(out, name, *a)
        else:
            assert kind == "attn"
            S._unet_attn(out, name, *a)
    for k, C in enumerate(ZERO_WIDTHS, start=1):
        S._conv(out, f"zero.skip{k}", C, C, 1)
    S._conv(out, "zero.mid", 1280, 1280, 1)
    n_plain = len(out)
    if torch:
        for i, (kind, a, _) in enumerate(steps, start=1):
            name = f"unet.layer{i}"
            if kind == "res":
                S._norm(out, name + ".layer1", a[0])
                S._norm(out, name + ".layer4", a[1])
            elif kind == "attn":
                for n in (1, 3, 5, 7):
                    S._norm(out, f"{name}.layer{n}", a[0] * a[1])
    return out, n_plain


@pytest.mark.parametrize("kind,torch", [("controlnet_sd15", False), ("controlnet_sd15_torch", True)])
def test_parameter_inventory(tsd_mod, kind, torch):
    want, n_plain = _expected(torch)
    got = tsd_mod.param_specs(kind)
    assert [g[0] for g in got] == [w.name for w in want]
    assert [g[1] for g in got] == [w.shape for w in want]
    assert [g[2] for g in got] == [w.used for w in want]
    zero_init = {f"hint.conv{len(HINT)}.kernel", "zero.mid.kernel"} | {f"zero.skip{k}.kernel" for k in range(1, 13)}
    for (name, _, _, bound), w in zip(got, want):
        assert bound == pytest.approx(0.0 if name in zero_init else w.bound, rel=1e-6), name
    # the pushes of the steps through the bottleneck are the twelve skips, in this order of widths
    pushed = [(a[0] * a[1] if k == "attn" else a[1]) for k, a, f in S.FULL_UNET_STEPS[:R.ENC_N] if f == "push"]
    assert tuple(pushed) == ZERO_WIDTHS
    if torch:   # norms appended last: the shared indices equal the plain kind's
        plain = tsd_mod.param_specs("controlnet_sd15")
        assert len(plain) == n_plain and got[:n_plain] == plain
        assert all(len(s) == 1 for _, s, _, _ in got[n_plain:])
    # the shared layers carry the UNet's own names and shapes
    unet = {n: s for n, s, _, _ in tsd_mod.param_specs("diffusion_sd15_torch" if torch else "diffusion_sd15")}
    shared = [(n, s) for n, s, _, _ in got if n.startswith(("unet.", "time_embed."))]
    assert shared and all(unet[n] == s for n, s in shared)
    assert tsd_mod._lib.lib().tsd_model_param_count(12) == tsd_mod._lib.TSD_E_ARG
    assert tsd_mod.flop_count(kind, 64) == -1.0


def test_diffusers_key_map_round_trip(tsd_mod):
    from tsd import checkpoint as ck
    specs = [(n, s) for n, s, used, _ in tsd_mod.param_specs("controlnet_sd15_torch") if used]
    P = {n: np.full(s, float(i + 1), np.float32) for i, (n, s) in enumerate(specs)}   # every tensor recognisable
    sd = ck.params_to_diffusers_controlnet(P)
    back = ck.diffusers_controlnet_to_params(sd)
    assert set(back) == set(P) and all(np.array_equal(back[n], P[n]) for n in P)
    own = {k for k in sd if k.startswith("controlnet_")}
    want = {f"controlnet_cond_embedding.{m}.{f}" for m in ["conv_in", "conv_out"] + [f"blocks.{i}" for i in range(6)] for f in ("weight", "bias")}
    want |= {f"controlnet_down_blocks.{i}.{f}" for i in range(12) for f in ("weight", "bias")}
    want |= {f"controlnet_mid_block.{f}" for f in ("weight", "bias")}
    assert own == want
    rest = sd.keys() - own   # the UNet encoder's names for the rest: a subset of the UNet map's keys, nothing of the decoder or the output layer
    unet_specs = {n: np.zeros(s, np.float32) for n, s, used, _ in tsd_mod.param_specs("diffusion_sd15_torch") if used}
    unet_keys = set(ck.params_to_diffusers_sd15_unet(unet_specs))
    assert rest <= unet_keys
    assert not [k for k in rest if k.startswith(("up_blocks", "conv_out", "conv_norm_out"))]
    assert {k.split(".")[0] for k in rest} == {"time_embedding", "conv_in", "down_blocks", "mid_block"}
    # the stacked q / k / v of self-attention come apart and back in order
    q = sd["down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q.weight"]
    assert q.shape == (320, 320)
    complete = ck.controlnet_params_complete(back)
    assert set(complete) == {n for n, _, _, _ in tsd_mod.param_specs("controlnet_sd15_torch")}
    with pytest.raises(KeyError):
        ck.controlnet_params_complete({k: v for k, v in back.items() if k != "zero.mid.kernel"})


def _cheap_params(specs, tag):
    """Every used parameter a scaled slice of ONE random buffer: the graph's 860 M parameters without drawing 860 M numbers."""
    big = max(int(np.prod(s)) for _, s, used, _ in specs if used)
    buf = rng.uniform(3, tag, big, 1.0)
    return {n: (buf[:int(np.prod(s))].reshape(s) * np.float32(b)) for n, s, used, b in specs if used}


def test_reference_with_zero_convolutions_is_the_plain_unet(tsd_mod):
    """At their zero initialisation the ControlNet's residuals are exactly zero, and the reference's controlled UNet is
    oracle.models.diffusion_sd15 exactly - with a non-zero residual it is not."""
    L = 16
    PC = _cheap_params(tsd_mod.param_specs("controlnet_sd15"), 1)
    PU = _cheap_params(tsd_mod.param_specs("diffusion_sd15"), 2)
    x = rng.normal(3, 10, 4 * L * L).reshape(4, L, L)
    ctx = rng.normal(3, 11, 77 * 768).reshape(77, 768)
    hint = rng.uniform(3, 12, 3 * 64 * L * L, 1.0).reshape(3, 8 * L, 8 * L)
    temb = ops.time_embedding(500.0)
    res = R.controlnet(PC, x, ctx, temb, hint)
    assert [r.shape for r in res] == [(320, 16, 16)] * 3 + [(320, 8, 8)] + [(640, 8, 8)] * 2 + [(640, 4, 4)] + [(1280, 4, 4)] * 2 + [(1280, 2, 2)] * 4
    assert all(not r.any() for r in res)
    plain = models.diffusion_sd15(PU, x, ctx, temb)
    np.testing.assert_array_equal(R.diffusion_sd15_controlled(PU, x, ctx, temb, res, 1.0), plain)
    np.testing.assert_array_equal(R.diffusion_sd15_controlled(PU, x, ctx, temb, None, 0.0), plain)
    res[12] = np.ones_like(res[12])
    assert not np.array_equal(R.diffusion_sd15_controlled(PU, x, ctx, temb, res, 1.0), plain)
    np.testing.assert_array_equal(R.diffusion_sd15_controlled(PU, x, ctx, temb, res, 0.0), plain)


def test_draw_params_gives_the_zero_convolutions_their_fan_in_bound(tsd_mod):
    specs = [(n, s, u, b) for n, s, u, b in tsd_mod.param_specs("controlnet_sd15_torch")
             if n.startswith(("zero.skip1.", "zero.mid.", "hint.conv8.", "hint.conv1.", "unet.layer2.layer1."))]
    P = R.draw_params(specs, 5, nonzero=("zero.", "hint.conv8"))
    for name, fan_in in (("zero.skip1.kernel", 320), ("zero.mid.kernel", 1280), ("hint.conv8.kernel", 256 * 9)):
        a = np.abs(P[name])
        assert 0.9 / np.sqrt(fan_in) < a.max() <= 1.0 / np.sqrt(fan_in)
    assert not P["zero.mid.bias"].any()
    assert not R.draw_params(specs, 5)["zero.mid.kernel"].any()
    assert abs(P["unet.layer2.layer1.weight"].mean() - 1.0) < 0.1   # norm weights are 1 + U


def test_library_exports_the_new_symbols(tsd_mod):
    declared = tsd_mod._lib.declared_symbols()
    lib = tsd_mod._lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/tsd.h"
        assert hasattr(lib, name), f"libtsd.so does not export {name}"
    assert not [n for n in declared if not hasattr(lib, n)]
    assert tsd_mod._lib.MODEL_CONTROLNET_SD15 == 10 and tsd_mod._lib.MODEL_CONTROLNET_SD15_TORCH == 11
    assert callable(tsd_mod.control_inject) and tsd_mod.ControlNet.__name__ == "ControlNet"


def test_generate_takes_the_control_keywords_and_generate_stream_refuses_them(tsd_mod):
    import inspect
    names = set(inspect.signature(tsd_mod.generate).parameters)
    assert {"controlnet", "control_image", "control_scale", "control_cond_only", "control_start", "control_end"} <= names
    assert {"set_control", "control_active"} <= set(dir(tsd_mod.Session)) and "hint" in dir(tsd_mod.ControlNet)
    with pytest.raises(ValueError):   # before anything touches a device
        next(iter(tsd_mod.generate_stream(None, None, [], 1, 16, controlnet=object(), control_image=np.zeros((3, 128, 128), np.float32))))
    with pytest.raises(ValueError):
        next(iter(tsd_mod.generate_stream(None, None, [], 1, 16, control_scale=0.5)))
    with pytest.raises(ValueError):   # controlnet and control_image go together
        tsd_mod.generate(None, None, np.zeros((1, 77, 768), np.float32), cfg=False, controlnet=object())
