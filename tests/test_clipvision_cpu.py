"""CPU: the CLIP vision encoder's kind number, inventory and FLOP count, the fp64 restatement of its image front end against PIL's float
resize, the size rule by hand, the encoder restatement against an independent torch restatement, the Hugging Face key map on synthetic
safetensors files, and `generate`'s argument checks.  No GPU: the inventory and the key map are host code, the references are numpy."""
import numpy as np
import pytest

import clipvision_ref as R
import replay

NEW_SYMBOLS = ("tsd_clip_image_patches_f16", "tsd_clip_vision_forward", "tsd_debug_image_patches_run")
SIZES = [(300, 500), (224, 224), (64, 96), (512, 512), (1024, 768), (225, 227)]   # (H, W)


def _image(H, W, seed):
    return np.random.default_rng(seed).uniform(0.0, 255.0, size=(3, H, W)).astype(np.float32)


# ---- the kind ---------------------------------------------------------------------------------------------------------------------------
def test_kind_number_header_and_reserved_numbers(tsd_mod):
    hdr = replay.header()
    assert tsd_mod.model.KINDS["clip_vision_h"] == 22 and "TSD_MODEL_CLIP_VISION_H = 22" in hdr
    lib = tsd_mod._lib.lib()
    for kind in (12, 13, 14, 15, 18, 19, 21, 23):            # still reserved or unknown
        assert lib.tsd_model_param_count(kind) == tsd_mod._lib.TSD_E_ARG, kind
    full = open(replay.HDR).read()
    assert "The CLIP vision encoder and the resampler" not in full and "tsd_clip_vision_forward below computes it from pixels" in full   # the sentence the encoder made untrue
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr and name in tsd_mod._lib.declared_symbols() and hasattr(lib, name), name
    for attr in ("CLIPVision", "clip_image_patches"):
        assert hasattr(tsd_mod, attr)
    from tsd import checkpoint as ck
    assert all(hasattr(ck, f) for f in ("load_clip_vision", "clip_vision_to_params", "params_to_clip_vision"))


def test_parameter_names_and_shapes(tsd_mod):
    got = [(n, tuple(s)) for n, s, _, _ in tsd_mod.param_specs("clip_vision_h")]
    want = R.reduced_specs(width=1280, layers=32, patch_k=588, tokens=257, mlp=5120, embed=1024)
    assert got == want and len(got) == 5 + 32 * 12 + 3
    assert all(used for _, _, used, _ in tsd_mod.param_specs("clip_vision_h"))
    assert sum(int(np.prod(s)) for _, s in got) == 632_076_800          # the 632 M parameters of ViT-H/14 with its projection


def test_flop_count_is_the_per_image_census(tsd_mod):
    T, D, F = 257, 1280, 5120
    lin = lambda m, k, n: 2.0 * m * k * n  # noqa: E731
    want = 32 * (lin(T, D, 3 * D) + lin(T, D, D) + lin(T, D, F) + lin(T, F, D) + 4.0 * T * T * D) + lin(256, 588, D) + lin(1, D, 1024)
    got = tsd_mod.flop_count("clip_vision_h", 0, 0)
    assert abs(got - want / 1e9) <= 1e-9 * want / 1e9 and 330 < got < 340
    assert tsd_mod.flop_count("clip_vision_h", 64, 77) == got               # L and T are not read


# ---- the front end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_resize_restatement_against_pil_float_mode(H, W):
    Image = pytest.importorskip("PIL.Image")
    img = _image(H, W, H * 7 + W)
    RH, RW = R.resized_size(H, W)
    top, left = R.crop_offsets(H, W)
    ref = np.stack([np.asarray(Image.fromarray(img[c], mode="F").resize((RW, RH), resample=Image.BICUBIC), np.float64)[top:top + 224, left:left + 224]
                    for c in range(3)])
    got = R.resize_crop(img)
    err = np.abs(got - ref).max()
    print(f"[clipvision] {H}x{W} -> {RH}x{RW}: max |restatement - PIL F| = {err:.3e}")
    assert err <= 255.0 * 2.0 ** -20


def test_identity_at_224_and_rows_sum_to_one():
    img = _image(224, 224, 3)
    assert np.array_equal(R.resize_crop(img), img.astype(np.float64))
    for H, W in SIZES + [(8, 8), (2048, 2048), (96, 64)]:
        wy, ty, wx, tx = R.tables(H, W)
        assert np.abs(wy.sum(1) - 1.0).max() < 1e-14 and np.abs(wx.sum(1) - 1.0).max() < 1e-14
        assert ty.max() <= 38 and tx.max() <= 38
    _, ty, _, tx = R.tables(2048, 2048)
    assert 37 <= ty.max() <= 38 and 37 <= tx.max() <= 38                    # the tap maximum of the accepted range: 2 * 2 * 2048 / 224 + 1
    taps = [int(t.max()) for H, W in SIZES for t in R.tables(H, W)[1::2]]
    assert min(taps) == 4 and max(taps) == 14                               # identity ... 1024 -> 298


def test_size_rule_by_hand():
    assert R.resized_size(300, 500) == (224, 373) and R.crop_offsets(300, 500) == (0, 74)
    assert R.resized_size(1024, 768) == (298, 224) and R.crop_offsets(1024, 768) == (37, 0)
    assert R.resized_size(225, 227) == (224, 225) and R.crop_offsets(225, 227) == (0, 0)
    assert R.resized_size(224, 224) == (224, 224)


def test_patch_layout_and_bound_shape():
    img = _image(64, 96, 1)
    ref, b = R.bound(img)
    y = R.normalise(R.resize_crop(img))
    assert ref.shape == b.shape == (256, 588)
    assert ref[3 * 16 + 5, 2 * 196 + 7 * 14 + 9] == y[2, 3 * 14 + 7, 5 * 14 + 9]
    assert (b > 0).all() and (b < 2.0 ** -10 * (np.abs(ref) + 1)).all()      # the fp16 half-ulp and a little: no loose envelope


# ---- the encoder restatement against torch, fp64 ----------------------------------------------------------------------------------------
def test_encoder_restatement_against_torch_fp64():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    width, heads, layers, n_patch, pk = 64, 2, 2, 9, 27
    g = np.random.default_rng(5)
    P = {n: (1.0 + 0.3 * g.standard_normal(s)) if (n.endswith(".weight") and len(s) == 1) else 0.2 * g.standard_normal(s)
         for n, s in R.reduced_specs(width, layers, pk, n_patch + 1, 128, 32)}
    rows = g.standard_normal((n_patch, pk))
    emb, hid = R.encoder(P, rows, heads, layers, np.float64)
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()}
    x = torch.tensor(rows, dtype=torch.float64) @ t["embeddings.patch_embedding.weight"].T
    x = torch.cat([t["embeddings.class_embedding"][None], x]) + t["embeddings.position_embedding.weight"]
    x = F.layer_norm(x, (width,), t["pre_layrnorm.weight"], t["pre_layrnorm.bias"], 1e-5)
    thid = None
    for i in range(layers):
        n = f"layers.{i}"
        thid = x
        h = F.layer_norm(x, (width,), t[n + ".ln1.weight"], t[n + ".ln1.bias"], 1e-5)
        q, k, v = (F.linear(h, t[n + ".in_proj.weight"], t[n + ".in_proj.bias"]).reshape(-1, 3, heads, width // heads).permute(1, 2, 0, 3))
        o = F.scaled_dot_product_attention(q[None], k[None], v[None])[0].permute(1, 0, 2).reshape(-1, width)
        x = x + F.linear(o, t[n + ".out_proj.weight"], t[n + ".out_proj.bias"])
        h = F.layer_norm(x, (width,), t[n + ".ln2.weight"], t[n + ".ln2.bias"], 1e-5)
        x = x + F.linear(F.gelu(F.linear(h, t[n + ".fc1.weight"], t[n + ".fc1.bias"])), t[n + ".fc2.weight"], t[n + ".fc2.bias"])
    temb = F.linear(F.layer_norm(x[:1], (width,), t["post_layernorm.weight"], t["post_layernorm.bias"], 1e-5), t["visual_projection.weight"])[0]
    e1, e2 = np.abs(emb - temb.numpy()).max(), np.abs(hid - thid.numpy()).max()
    print(f"[clipvision] encoder restatement vs torch fp64: embeds {e1:.2e}, hidden {e2:.2e}")
    assert emb.shape == (32,) and hid.shape == (n_patch + 1, width) and e1 <= 1e-10 and e2 <= 1e-10


# ---- the key map ------------------------------------------------------------------------------------------------------------------------
def _hf_state(layers=2, width=1280, seed=0):
    g = np.random.default_rng(seed)
    r = lambda *s: (0.02 * g.standard_normal(s)).astype(np.float32)  # noqa: E731
    vm = "vision_model."
    st = {vm + "embeddings.class_embedding": r(width), vm + "embeddings.patch_embedding.weight": r(width, 3, 14, 14),
          vm + "embeddings.position_embedding.weight": r(257, width), vm + "embeddings.position_ids": np.arange(257, dtype=np.float32)[None],
          vm + "pre_layrnorm.weight": r(width), vm + "pre_layrnorm.bias": r(width)}
    for i in range(layers):
        h = vm + f"encoder.layers.{i}."
        for m, (o, k) in {"layer_norm1": (width, None), "layer_norm2": (width, None), "self_attn.q_proj": (width, width), "self_attn.k_proj": (width, width),
                          "self_attn.v_proj": (width, width), "self_attn.out_proj": (width, width), "mlp.fc1": (4 * width, width),
                          "mlp.fc2": (width, 4 * width)}.items():
            st[h + m + ".weight"] = r(o) if k is None else r(o, k)
            st[h + m + ".bias"] = r(o)
    st[vm + "post_layernorm.weight"], st[vm + "post_layernorm.bias"] = r(width), r(width)
    st["visual_projection.weight"] = r(1024, width)
    return st


def test_key_map_round_trip_on_a_synthetic_file(tsd_mod, tmp_path):
    from tsd import checkpoint as ck
    st = _hf_state(2, seed=1)
    path = str(tmp_path / "image_encoder.safetensors")
    ck.write_safetensors(path, st)
    params = ck.clip_vision_to_params(ck.read_safetensors(path))
    specs = {n: tuple(s) for n, s, _, _ in tsd_mod.param_specs("clip_vision_h")}
    assert set(params) == {n for n in specs if not n.startswith("layers.") or int(n.split(".")[1]) < 2}
    assert all(params[n].shape == specs[n] for n in params)
    vm = "vision_model."
    assert np.array_equal(params["layers.1.in_proj.weight"][1280:2560], st[vm + "encoder.layers.1.self_attn.k_proj.weight"])
    assert np.array_equal(params["embeddings.patch_embedding.weight"][7, 2 * 196 + 3 * 14 + 5], st[vm + "embeddings.patch_embedding.weight"][7, 2, 3, 5])
    back = ck.params_to_clip_vision(params)
    want = {k: v for k, v in st.items() if not k.endswith("position_ids")}
    assert set(back) == set(want) and all(np.array_equal(back[k], want[k]) for k in want)


def test_refusals_of_the_key_map(tsd_mod):
    from tsd import checkpoint as ck
    st = _hf_state(1, seed=2)
    del st["vision_model.encoder.layers.0.mlp.fc2.bias"]
    with pytest.raises(ValueError, match=r"vision_model\.encoder\.layers\.0\.mlp\.fc2\.bias"):
        ck.clip_vision_to_params(st)
    st = _hf_state(1, seed=3)
    del st["visual_projection.weight"]
    with pytest.raises(ValueError, match=r"visual_projection\.weight"):
        ck.clip_vision_to_params(st)
    with pytest.raises(ValueError, match="1024 wide"):                      # a ViT-L/14 tower
        ck.clip_vision_to_params({"vision_model.embeddings.class_embedding": np.zeros(1024, np.float32)})
    with pytest.raises(ValueError, match=r"layers\.2\."):                  # 2 of 32 layers: refused before any device call, by name
        ck.load_clip_vision(_hf_state(2, seed=4))


# ---- generate's argument checks (raised before anything touches the device) ---------------------------------------------------------------
def test_generate_argument_checks(tsd_mod):
    ctx = np.zeros((1, 77, 768), np.float32)
    img = np.zeros((3, 32, 32), np.float32)
    with pytest.raises(ValueError, match="not both"):
        tsd_mod.generate(None, None, ctx, ip_adapter=object(), ip_image=img, ip_image_embeds=np.zeros(1024, np.float32), image_encoder=object())
    with pytest.raises(ValueError, match="image_encoder"):
        tsd_mod.generate(None, None, ctx, ip_adapter=object(), ip_image=img)
    with pytest.raises(ValueError, match="ip_adapter"):
        tsd_mod.generate(None, None, ctx, ip_image=img, image_encoder=object())
    with pytest.raises(ValueError, match="ip_adapter"):
        tsd_mod.generate(None, None, ctx, ip_adapter=object())
    import inspect
    doc = inspect.getdoc(tsd_mod.generate)
    assert "the vision encoder is not part of this package" not in doc and "image_encoder" in doc
