"""CPU: the IP-Adapter kind's parameter inventory, the published key map (round trip and the wrong-order refusal on synthetic safetensors
files), the reference module's own consistency (the emulation of the kernel's rounding points inside the derived bound) and the exported
symbols.  No GPU: the inventory and the key map are host code, the reference is numpy."""
import numpy as np
import pytest

import ipadapter_ref as R
import replay
from oracle import spec as S

NEW_SYMBOLS = ("tsd_ip_adapter_project", "tsd_diffusion_forward_ip_hw", "tsd_ip_attn_add_f16", "tsd_session_set_ip_adapter",
               "tsd_session_ip_adapter_active", "tsd_debug_ip_attn_run", "tsd_debug_ip_attn_bench")
TABLE_WIDTHS = (320, 320, 640, 640, 1280, 1280, 1280) + (1280,) * 3 + (640,) * 3 + (320,) * 3   # 6 down, mid, 9 up


def test_parameter_inventory(tsd_mod):
    got = tsd_mod.param_specs("ip_adapter_sd15")
    assert tsd_mod.model.KINDS["ip_adapter_sd15"] == 20 and "TSD_MODEL_IP_ADAPTER_SD15 = 20" in replay.header()
    names = [g[0] for g in got]
    assert names[:4] == ["image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias"]
    assert [tuple(g[1]) for g in got[:4]] == [(4 * 768, 1024), (4 * 768,), (768,), (768,)]
    # the 16 pairs in the step table's order, under the published files' numbers, no bias entries
    widths = tuple(a[0] * a[1] for kind, a, _ in S.FULL_UNET_STEPS if kind == "attn")
    assert widths == TABLE_WIDTHS
    want = []
    for t, C in enumerate(widths):
        for f in ("to_k_ip", "to_v_ip"):
            want.append((f"ip_adapter.{R.published_index(t)}.{f}.weight", (C, 768)))
    assert [(g[0], tuple(g[1])) for g in got[4:]] == want and len(got) == 36
    assert sorted(R.published_index(t) for t in range(16)) == list(range(1, 32, 2))
    assert all(g[2] for g in got)                        # every parameter is read
    assert sum(C for C in widths) == 12480
    lib = tsd_mod._lib.lib()
    assert lib.tsd_model_param_count(20) == 36
    for kind in (12, 13, 14, 15, 18, 19, 21):            # still reserved or unknown
        assert lib.tsd_model_param_count(kind) == tsd_mod._lib.TSD_E_ARG
    assert tsd_mod.flop_count("ip_adapter_sd15", 64) == -1.0


def _published_state(seed=0, widths=None):
    from tsd import checkpoint as ck
    r = np.random.default_rng(seed)
    st = {"image_proj.proj.weight": r.standard_normal((4 * 768, 1024)).astype(np.float32) * 0.02,
          "image_proj.proj.bias": r.standard_normal(4 * 768).astype(np.float32) * 0.02,
          "image_proj.norm.weight": (1 + 0.1 * r.standard_normal(768)).astype(np.float32),
          "image_proj.norm.bias": (0.1 * r.standard_normal(768)).astype(np.float32)}
    for k, C in enumerate(widths or ck.IP_ADAPTER_PUBLISHED_WIDTHS):
        for f in ("to_k_ip", "to_v_ip"):
            st[f"ip_adapter.{2 * k + 1}.{f}.weight"] = r.standard_normal((C, 768)).astype(np.float32) * 0.03
    return st


def test_published_key_map_round_trip_on_a_synthetic_file(tsd_mod, tmp_path):
    from tsd import checkpoint as ck
    st = _published_state(1)
    path = str(tmp_path / "ip-adapter_sd15.safetensors")
    ck.write_safetensors(path, st)
    params = ck.ip_adapter_to_params(ck.read_safetensors(path))
    specs = {n: tuple(s) for n, s, _, _ in tsd_mod.param_specs("ip_adapter_sd15")}
    assert set(params) == set(specs) and all(params[n].shape == specs[n] for n in specs)
    # the published order is down, up, mid: published k = 15 (index 31) is the step table's block 6, k = 6 (index 13) its block 7
    assert R.published_index(6) == 31 and R.published_index(7) == 13
    assert np.array_equal(params["ip_adapter.31.to_k_ip.weight"], st["ip_adapter.31.to_k_ip.weight"])
    back = ck.params_to_ip_adapter(params)
    assert list(back) == list(st) and all(np.array_equal(back[k], st[k]) for k in st)


def test_a_file_with_another_width_order_is_refused(tsd_mod, tmp_path):
    """down, MID, up instead of down, up, mid: the same tensors under other numbers must not load silently."""
    from tsd import checkpoint as ck
    w = ck.IP_ADAPTER_PUBLISHED_WIDTHS
    wrong = w[:6] + (w[15],) + w[6:15]
    assert sorted(wrong) == sorted(w) and wrong != w
    path = str(tmp_path / "wrong.safetensors")
    ck.write_safetensors(path, _published_state(2, wrong))
    with pytest.raises(ValueError, match="widths"):
        ck.ip_adapter_to_params(ck.read_safetensors(path))
    st = _published_state(3)
    del st["ip_adapter.7.to_v_ip.weight"]
    with pytest.raises(KeyError):
        ck.ip_adapter_to_params(st)
    with pytest.raises(KeyError, match="plus"):
        ck.load_ip_adapter({"image_proj.latents": np.zeros((1, 16, 768), np.float32)})


CASES = [(hd, N, S) for hd in (40, 80, 160) for N, S in ((1, 4), (4, 16), (5, 48), (16, 80))]


@pytest.mark.parametrize("hd,N,S", CASES)
def test_emulation_of_the_kernels_rounding_points_is_inside_the_bound(hd, N, S):
    d = R.desc(3, 8, hd, S, N)
    ops = R.make_inputs(d, seed=hd + N, scales=[0.0, 1.0, 0.37])
    assert R.well_conditioned(d, ops)
    ref, b = R.reference(d, ops), R.bound(d, ops)
    err = np.abs(R.emulate(d, ops).astype(np.float64) - ref)
    assert (err <= b).all(), f"emulation outside the bound: worst ratio {(err / np.maximum(b, 1e-300)).max():.3f}"
    q, k, vt, o, s = R.unpack(d, ops)
    assert np.array_equal(R.emulate(d, ops)[0].view(np.uint16), o[0].view(np.uint16)) and (b[0] == 0).all()   # scale 0: untouched
    # the bound is about the output rounding plus a small multiple of it, not a loose envelope
    assert b[1:].max() < 8 * R.U16 * (np.abs(ref[1:]).max() + 1)


def test_bound_holds_over_the_fp16_exponent_range_of_p_and_a_negative_scale():
    d = R.desc(2, 8, 40, 16, 16)
    ops = R.make_inputs(d, seed=5, scales=[1.0, -0.8], span=22.0)   # exp(-22) = 2.8e-10: far below the smallest fp16 subnormal
    assert not R.well_conditioned(d, ops)
    q, k, v, o, s = R._heads(d, ops, np.float64)
    z = R.scale_of(d) * (q @ k.transpose(0, 1, 3, 2))
    assert (z.max(-1) - z.min(-1)).min() > 17.4, "the smallest p must underflow to 0 in fp16"
    err = np.abs(R.emulate(d, ops).astype(np.float64) - R.reference(d, ops))
    assert (err <= R.bound(d, ops)).all()


def test_mutated_emulations_leave_the_bound():
    """The bound separates the kernel from near misses: an unmasked pad key, a softmax scale of the wrong head dimension."""
    d = R.desc(1, 8, 80, 16, 5)
    ops = R.make_inputs(d, seed=9)
    ref, b = R.reference(d, ops), R.bound(d, ops)
    d6 = d.copy(); d6[R.PD["N"]] = 6          # admits key 5: a zero key, score 0, with a zero value
    assert (np.abs(R.emulate(d6, ops).astype(np.float64) - ref) > b).any()
    ds = d.copy(); ds[R.PD["SCALE"]] = replay.f32_bits(1.0 / np.sqrt(40.0))
    assert (np.abs(R.emulate(ds, ops).astype(np.float64) - ref) > b).any()


def test_descriptor_sizing_needs_no_device():
    d = R.desc(3, 8, 40, 48, 4)
    rc, ext = replay.size("tsd_debug_ip_attn_run", d)
    assert rc == 0 and {s: int(ext[R.PO[s]]) for s in R.extents(d)} == R.extents(d)
    bad = d.copy(); bad[R.PD["VERSION"]] = 9
    assert replay.size("tsd_debug_ip_attn_run", bad)[0] != 0
    bad = d.copy(); bad[R.PD["LDVT"]] = 8     # V^T needs its 16 columns
    assert replay.size("tsd_debug_ip_attn_run", bad)[0] != 0


def test_new_entries_are_declared_bound_and_exported(tsd_mod):
    hdr = replay.header()
    declared = tsd_mod._lib.declared_symbols()
    lib = tsd_mod._lib.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, f"{name} is not declared in include/tsd.h"
        assert name in declared, f"{name} is not bound in tsd/_lib.py"
        assert hasattr(lib, name), f"libtsd.so does not export {name}"
    for attr in ("IPAdapter", "ip_attn_add"):
        assert hasattr(tsd_mod, attr)
    assert hasattr(tsd_mod.Session, "set_ip_adapter") and hasattr(tsd_mod.checkpoint if hasattr(tsd_mod, "checkpoint") else __import__("tsd.checkpoint").checkpoint, "load_ip_adapter")


def test_generate_stream_refuses_the_adapter_keywords(tsd_mod):
    with pytest.raises(ValueError, match="IP-Adapter"):
        next(tsd_mod.generate_stream(None, None, iter(()), 1, 16, ip_adapter=object(), ip_image_embeds=np.zeros(1024, np.float32)))
    with pytest.raises(ValueError, match="IP-Adapter"):
        next(tsd_mod.generate_stream(None, None, iter(()), 1, 16, ip_scale=0.5))
