"""CPU: the IP-Adapter Plus kind's parameter inventory, the plus key map (round trip and refusals on synthetic safetensors files), the
reference module's own separation of the near misses, the exported symbols, the keyword refusals of `generate` / `generate_stream` and
the neutral image.  No GPU: the inventory and the key map are host code, the reference is numpy."""
import inspect

import numpy as np
import pytest

import clipvision_ref as CV
import ipplus_ref as R
import replay
from oracle import spec as S
from util import TOL_MODEL, rel_l2

NEW_SYMBOLS = ("tsd_ip_adapter_resample",)
KIND = "ip_adapter_plus_sd15"


def test_parameter_inventory(tsd_mod):
    got = tsd_mod.param_specs(KIND)
    hdr = replay.header()
    assert tsd_mod.model.KINDS[KIND] == 24 and "TSD_MODEL_IP_ADAPTER_PLUS_SD15 = 24" in hdr
    assert "TSD_MODEL_IP_ADAPTER_SD15 = 20" in hdr and "TSD_MODEL_CLIP_VISION_H = 22" in hdr
    want = R.inventory()
    assert len(want) == R.N_PARAMS == 83 and [(g[0], tuple(g[1])) for g in got] == want
    assert [n for n, _ in want[:7]] == ["image_proj.latents", "image_proj.proj_in.weight", "image_proj.proj_in.bias", "image_proj.proj_out.weight",
                                        "image_proj.proj_out.bias", "image_proj.norm_out.weight", "image_proj.norm_out.bias"]
    assert want[0][1] == (1, 16, 768) and want[1][1] == (768, 1280) and want[12][1] == (1536, 768) and want[17][1] == (768, 3072)
    assert sum(int(np.prod(s)) for _, s in want) == R.N_ELEMENTS == 49087488
    assert sum(int(np.prod(s)) for n, s in want if n.startswith("image_proj.")) == R.N_ELEMENTS_IMAGE_PROJ == 29918208
    # the 32 pair entries are exactly kind 20's, name for name and shape for shape, in the step table's order
    assert [(g[0], tuple(g[1])) for g in got[51:]] == [(g[0], tuple(g[1])) for g in tsd_mod.param_specs("ip_adapter_sd15")[4:]]
    assert tuple(a[0] * a[1] for kind, a, _ in S.FULL_UNET_STEPS if kind == "attn") == R.TABLE_WIDTHS
    assert all(g[2] for g in got)                        # every parameter is read
    lib = tsd_mod._lib.lib()
    assert lib.tsd_model_param_count(24) == 83 and lib.tsd_model_param_count(20) == 36
    for kind in (12, 13, 14, 15, 18, 19, 21, 23):        # still reserved and refused
        assert lib.tsd_model_param_count(kind) == tsd_mod._lib.TSD_E_ARG
    assert tsd_mod.flop_count(KIND, 64) == tsd_mod.flop_count("ip_adapter_sd15", 64) == -1.0


def _plus_state(seed=0, widths=None, latents=(1, 16, 768), embed=1280):
    """A synthetic plus file: the published names, the 16 pairs in the published order."""
    from tsd import checkpoint as ck
    r = np.random.default_rng(seed)
    shapes = dict(R.inventory())
    st = {}
    for n in ck.ip_adapter_plus_names():
        if n.startswith("ip_adapter."):
            continue
        shape = latents if n == "image_proj.latents" else ((768, embed) if n == "image_proj.proj_in.weight" else shapes[n])
        st[n] = (0.03 * r.standard_normal(shape)).astype(np.float32)
    for k, C in enumerate(widths or ck.IP_ADAPTER_PUBLISHED_WIDTHS):
        for f in ("to_k_ip", "to_v_ip"):
            st[f"ip_adapter.{2 * k + 1}.{f}.weight"] = (0.03 * r.standard_normal((C, 768))).astype(np.float32)
    return st


def test_plus_key_map_round_trip_on_a_synthetic_file(tsd_mod, tmp_path):
    from tsd import checkpoint as ck
    st = _plus_state(1)
    assert len(st) == 83
    path = str(tmp_path / "ip-adapter-plus_sd15.safetensors")
    ck.write_safetensors(path, st)
    params = ck.ip_adapter_plus_to_params(ck.read_safetensors(path))
    specs = {n: tuple(s) for n, s, _, _ in tsd_mod.param_specs(KIND)}
    assert set(params) == set(specs) and all(params[n].shape == specs[n] for n in specs)
    assert np.array_equal(params["image_proj.layers.2.0.to_kv.weight"], st["image_proj.layers.2.0.to_kv.weight"])
    assert np.array_equal(params["ip_adapter.31.to_k_ip.weight"], st["ip_adapter.31.to_k_ip.weight"])
    back = ck.params_to_ip_adapter_plus(params)
    assert list(back) == list(st) and all(np.array_equal(back[k], st[k]) for k in st)


def test_the_loaders_refusals(tsd_mod):
    from tsd import checkpoint as ck
    st = _plus_state(2)
    del st["image_proj.layers.3.1.3.weight"]
    with pytest.raises(KeyError, match=r"image_proj\.layers\.3\.1\.3\.weight"):       # a missing tensor, by name
        ck.load_ip_adapter_plus(st)
    w = ck.IP_ADAPTER_PUBLISHED_WIDTHS
    wrong = w[:6] + (w[15],) + w[6:15]                                                 # down, MID, up
    with pytest.raises(ValueError, match="widths"):
        ck.load_ip_adapter_plus(_plus_state(3, widths=wrong))
    with pytest.raises(ValueError, match=r"latents.*\(1, 257, 768\)"):
        ck.load_ip_adapter_plus(_plus_state(4, latents=(1, 257, 768)))
    with pytest.raises(ValueError, match=r"latents.*\(1, 16, 1280\)"):
        ck.load_ip_adapter_plus(_plus_state(4, latents=(1, 16, 1280)))
    with pytest.raises(ValueError, match=r"proj_in.*\(768, 1024\)"):                   # a ViT-L tower
        ck.load_ip_adapter_plus(_plus_state(5, embed=1024))
    plain = {"image_proj.proj.weight": np.zeros((4 * 768, 1024), np.float32), "image_proj.proj.bias": np.zeros(4 * 768, np.float32)}
    with pytest.raises(KeyError, match="load_ip_adapter reads it"):                    # a kind-20 file
        ck.load_ip_adapter_plus(plain)
    with pytest.raises(KeyError, match="plus"):                                        # and the other way round, pointing here
        ck.load_ip_adapter({"image_proj.latents": np.zeros((1, 16, 768), np.float32)})
    assert "from memory" in inspect.getdoc(ck.ip_adapter_plus_to_params).lower()
    assert "load_ip_adapter_plus" in inspect.getdoc(ck.load_ip_adapter)


@pytest.fixture(scope="module")
def draw():
    return R.f16_weights(R.draw_params(3))


@pytest.mark.parametrize("S_", (5, 49))
def test_every_near_miss_is_far_from_the_reference(draw, S_):
    """What keeps the GPU test meaningful: each restatement one slip away is more than 10 TOL_MODEL from the module on the test draw."""
    h = R.hidden_states(1, S_, 4100 + S_)[0]
    spreads = []
    ref = R.resample(draw, h, spreads=spreads)
    assert ref.shape == (16, 768) and np.isfinite(ref).all()
    print(f"[ipplus] S = {S_}: smallest per-row score spread {min(spreads):.2f}")
    assert min(spreads) > 0.5, "the attention of the test draw is close to uniform: it would hide a wrong key set"
    for miss in R.NEAR_MISSES:
        e = rel_l2(R.resample(draw, h, miss), ref)
        print(f"[ipplus] S = {S_}: {miss} moves the result by {e:.3f} relative L2")
        assert e > 10 * TOL_MODEL, (miss, e)


def test_rounding_the_weights_to_fp16_moves_the_result_far_less_than_the_tolerance():
    P = R.draw_params(3)
    h = R.hidden_states(1, 49, 4149)[0]
    e = rel_l2(R.resample(R.f16_weights(P), h), R.resample(P, h))
    print(f"[ipplus] fp16 weights against fp32 weights: {e:.2e} relative L2")
    assert e < TOL_MODEL / 5


def test_new_entries_are_declared_bound_and_exported(tsd_mod):
    hdr = replay.header()
    declared = tsd_mod._lib.declared_symbols()
    lib = tsd_mod._lib.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, f"{name} is not declared in include/tsd.h"
        assert name in declared, f"{name} is not bound in tsd/_lib.py"
        assert hasattr(lib, name), f"libtsd.so does not export {name}"
    import os
    shim = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(tsd_mod.__file__))), "mojo_shim", "tsd_ffi.mojo")).read()
    assert "TSD_MODEL_IP_ADAPTER_PLUS_SD15: Int32 = 24" in shim and '"tsd_ip_adapter_resample"' in shim
    from tsd import checkpoint as ck
    for fn in ("ip_adapter_plus_to_params", "params_to_ip_adapter_plus", "load_ip_adapter_plus"):
        assert hasattr(ck, fn)
    assert hasattr(tsd_mod, "clip_neutral_image") and hasattr(tsd_mod.IPAdapter, "resample")
    assert tsd_mod.IPAdapter.VARIANTS == {"ip_adapter_sd15": 4, KIND: 16}
    # the sentences that said the resampler is no part of the library are gone; the phrases other tests pin are still there
    full = open(replay.HDR).read()
    assert "tsd_clip_vision_forward below computes it from pixels" in full
    assert 'The resampler of the "plus" files is not part of it' not in full and "TSD_E_NONFINITE - the convention" in full


class _Plus:       # what generate looks at before it touches a device
    is_plus = True


class _Plain:
    is_plus = False


def test_generate_keyword_refusals(tsd_mod):
    ctx = np.zeros((1, 77, 768), np.float32)
    hid = np.zeros((257, 1280), np.float32)
    g = tsd_mod.generate
    with pytest.raises(ValueError, match="plus adapter reads"):                        # embeds into a plus adapter
        g(None, None, ctx, ip_adapter=_Plus(), ip_image_embeds=np.zeros(1024, np.float32))
    with pytest.raises(ValueError, match="ip_hidden is what a plus adapter reads"):    # hidden states into a plain one
        g(None, None, ctx, ip_adapter=_Plain(), ip_hidden=hid)
    with pytest.raises(ValueError, match="ip_uncond_hidden"):                          # CFG without the unconditional half
        g(None, None, ctx, ip_adapter=_Plus(), ip_hidden=hid, cfg=True)
    with pytest.raises(ValueError, match="ip_adapter"):
        g(None, None, ctx, ip_hidden=hid)
    with pytest.raises(ValueError, match="not both"):
        g(None, None, ctx, ip_adapter=_Plus(), ip_hidden=hid, ip_image=np.zeros((3, 32, 32), np.float32), image_encoder=object())
    with pytest.raises(ValueError, match=r"\(S, 1280\)"):
        g(None, None, ctx, ip_adapter=_Plus(), ip_hidden=np.zeros((257, 1024), np.float32), cfg=False)
    with pytest.raises(ValueError, match="goes with ip_hidden"):
        g(None, None, ctx, ip_adapter=_Plus(), ip_uncond_hidden=hid, ip_image=np.zeros((3, 32, 32), np.float32), image_encoder=object())
    doc = inspect.getdoc(g)
    assert "ip_hidden" in doc and "clip_neutral_image" in doc and "subnormal" in doc


def test_generate_stream_refuses_the_new_keywords(tsd_mod):
    for kw in (dict(ip_hidden=np.zeros((257, 1280), np.float32)), dict(ip_uncond_hidden=np.zeros((257, 1280), np.float32))):
        with pytest.raises(ValueError, match="IP-Adapter"):
            next(tsd_mod.generate_stream(None, None, iter(()), 1, 16, **kw))


def test_neutral_image_normalises_to_zero_within_one_fp16_subnormal(tsd_mod):
    img = tsd_mod.clip_neutral_image()
    assert img.shape == (3, 224, 224) and img.dtype == np.float32
    assert all((img[c] == img[c, 0, 0]).all() for c in range(3))
    rows = CV.patches(img)                                   # the front end's fp64 restatement: identity resize, normalise, patch layout
    worst = float(np.abs(rows).max())
    print(f"[ipplus] neutral image through the front-end restatement: max |x| = {worst:.2e} (one fp16 subnormal is {2.0 ** -24:.2e})")
    assert rows.shape == (256, 588) and worst <= 2.0 ** -24
    assert "subnormal" in inspect.getdoc(tsd_mod.clip_neutral_image)
