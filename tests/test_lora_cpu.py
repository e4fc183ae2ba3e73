"""LoRA adapters, the part that needs no GPU: both key dialects parse to the same list, every adapter-carrying module of the SD-1.x
UNet and text encoder maps to rows of one of our parameters, bad files are refused before anything is applied, the new C entries
are declared, exported and bound and refuse NULL handles, and the float64 reference the GPU tests use rounds as they assume."""
import ctypes as C

import numpy as np
import pytest

from lora_ref import (ATTN_SUFFIXES, NEW_ENTRIES, as_state, attention_modules, check_interval, exact_operands, gamma,
                      general_operands, unet_pairs)

UNDERSCORED = "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_out.0"


def test_new_entries_are_declared_exported_and_bound(tsd_mod):
    lib = tsd_mod._lib.lib()
    declared = tsd_mod._lib.declared_symbols()
    for name, nargs in NEW_ENTRIES.items():
        assert name in declared, name
        fn = getattr(lib, name)          # AttributeError: not exported
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
    for name in ("read_lora", "lora_targets", "load_lora", "merge_reference"):
        assert callable(getattr(tsd_mod, name))
    for name in ("get_param", "packed_param", "lora_add", "lora_clear"):
        assert callable(getattr(tsd_mod.Model, name))
    assert isinstance(tsd_mod.Model.lora_count, property)


def test_entries_refuse_null_handles_without_a_device(tsd_mod):
    from tsd._lib import TSD_E_ARG, ptr
    lib = tsd_mod._lib.lib()
    a = np.zeros(4, np.float32)
    assert lib.tsd_model_lora_add(None, 0, 0, 1, ptr(a), ptr(a), 1, 1.0) == TSD_E_ARG
    assert lib.tsd_model_lora_clear(None) == TSD_E_ARG
    assert lib.tsd_model_lora_count(None) == TSD_E_ARG
    assert lib.tsd_model_get_param(None, 0, ptr(a), 4) == TSD_E_ARG
    assert lib.tsd_debug_model_packed_param(None, 0, None, 0) == TSD_E_ARG
    assert lib.tsd_lora_merge_f32(None, ptr(a), 1, 1, 0, 0, 0, 1, ptr(a), ptr(a), 1, 1.0, ptr(a)) == TSD_E_ARG
    # arguments are checked before the context is touched: a context that is no context (zeroed memory) must not be dereferenced
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for args in ((None, ptr(a), ptr(a), ptr(a)), (ptr(a), None, ptr(a), ptr(a)), (ptr(a), ptr(a), None, ptr(a)), (ptr(a), ptr(a), ptr(a), None)):
        assert lib.tsd_lora_merge_f32(ctx, args[0], 1, 1, 0, 0, 0, 1, args[1], args[2], 1, 1.0, args[3]) == TSD_E_ARG
    for rank in (0, -1, 1025):
        assert lib.tsd_lora_merge_f32(ctx, ptr(a), 1, 1, 0, 0, 0, 1, ptr(a), ptr(a), rank, 1.0, ptr(a)) == TSD_E_ARG, rank
    for scale in (np.inf, -np.inf, np.nan):
        assert lib.tsd_lora_merge_f32(ctx, ptr(a), 1, 1, 0, 0, 0, 1, ptr(a), ptr(a), 1, scale, ptr(a)) == TSD_E_ARG, scale
    assert lib.tsd_lora_merge_f32(ctx, ptr(a), 1, 1, 2, 0, 0, 1, ptr(a), ptr(a), 1, 1.0, ptr(a)) == TSD_E_ARG       # 2x2 kernel
    assert lib.tsd_lora_merge_f32(ctx, ptr(a), 3, 1, 0, 1, 0, 1, ptr(a), ptr(a), 1, 1.0, ptr(a)) == TSD_E_ARG       # interleave, odd rows
    from tsd._lib import TSD_E_SHAPE
    for row0, rows in ((0, 3), (2, 1), (-1, 1), (0, 0)):
        assert lib.tsd_lora_merge_f32(ctx, ptr(a), 2, 2, 0, 0, row0, rows, ptr(a), ptr(a), 1, 1.0, ptr(a)) == TSD_E_SHAPE, (row0, rows)


def _some_pairs(tsd_mod):
    mods = [UNDERSCORED, "down_blocks.1.attentions.0.proj_in", "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj",
            "up_blocks.0.resnets.1.conv1", "conv_in", "up_blocks.3.attentions.2.transformer_blocks.0.attn1.to_k",
            "down_blocks.0.resnets.0.time_emb_proj"]
    return unet_pairs(tsd_mod, mods, rank=4, seed=11)


def test_kohya_and_peft_files_parse_to_the_same_list(tsd_mod, tmp_path):
    from tsd.checkpoint import write_safetensors
    pairs = _some_pairs(tsd_mod)
    g = np.random.default_rng(5)
    te = {"text_model.encoder.layers.3.self_attn.k_proj": ((0.1 * g.standard_normal((2, 768))).astype(np.float32),
                                                            (0.1 * g.standard_normal((768, 2))).astype(np.float32)),
          "text_model.encoder.layers.11.mlp.fc1": ((0.1 * g.standard_normal((2, 768))).astype(np.float32),
                                                   (0.1 * g.standard_normal((3072, 2))).astype(np.float32))}
    lists = []
    for dialect in ("kohya", "peft"):
        st = as_state(pairs, dialect, alpha=2.0)
        st.update(as_state(te, dialect, alpha=1.0, prefix="text_encoder"))
        path = str(tmp_path / f"{dialect}.safetensors")
        write_safetensors(path, st)
        lists.append(tsd_mod.read_lora(path))
    a, b = lists
    assert len(a) == len(pairs) + len(te) and [x[0] for x in a] == [x[0] for x in b] == sorted(x[0] for x in a)
    for (ma, da, ua, aa), (mb, db, ub, ab) in zip(a, b):
        assert ma == mb and aa == ab and da.shape == db.shape and ua.shape == ub.shape
        assert da.tobytes() == db.tobytes() and ua.tobytes() == ub.tobytes(), ma
    got = {m: (d, u, al) for m, d, u, al in a}
    d, u, al = got["unet." + UNDERSCORED]   # the underscore form of this path splits nine ways; the table finds the one module
    assert al == 2.0 and d.tobytes() == pairs[UNDERSCORED][0].tobytes() and u.tobytes() == pairs[UNDERSCORED][1].tobytes()
    assert got["unet.up_blocks.0.resnets.1.conv1"][0].shape == (4, 2560, 3, 3) and got["unet.up_blocks.0.resnets.1.conv1"][1].shape == (1280, 4, 1, 1)
    assert got["text_encoder.text_model.encoder.layers.11.mlp.fc1"][2] == 1.0
    # the older diffusers spelling, the text encoder without its `text_model.` prefix, and a file without alpha
    st = {"unet.conv_in.lora.down.weight": pairs["conv_in"][0], "unet.conv_in.lora.up.weight": pairs["conv_in"][1],
          "text_encoder.encoder.layers.3.self_attn.k_proj.lora_A.weight": te["text_model.encoder.layers.3.self_attn.k_proj"][0],
          "text_encoder.encoder.layers.3.self_attn.k_proj.lora_B.weight": te["text_model.encoder.layers.3.self_attn.k_proj"][1]}
    got = tsd_mod.read_lora(st)
    assert [(m, al) for m, _, _, al in got] == [("text_encoder.text_model.encoder.layers.3.self_attn.k_proj", None), ("unet.conv_in", None)]


def test_every_unet_module_maps_to_rows_of_one_parameter(tsd_mod):
    from tsd.checkpoint import SD15_MODULES
    specs = {n: (s, used) for n, s, used, _ in tsd_mod.param_specs("diffusion_sd15_torch")}
    targets = tsd_mod.lora_targets("diffusion_sd15_torch")
    seen = set()
    for mod, (pname, row0, rows) in targets.items():
        shape, used = specs[pname]
        assert used and len(shape) in (2, 4) and row0 >= 0 and rows > 0 and row0 + rows <= shape[0], (mod, pname, row0, rows, shape)
        seen.add(pname)
    # every module of the flat layer list carries its adapters: the plain convs, the resnets' three / four matrices, the attention blocks' twelve
    for mod in SD15_MODULES:
        if ".attentions." in mod:
            for s in ATTN_SUFFIXES:
                assert f"{mod}.{s}" in targets, (mod, s)
        elif ".resnets." in mod:
            for s in ("conv1", "time_emb_proj", "conv2"):
                assert f"{mod}.{s}" in targets, (mod, s)
            cin, cout = specs[targets[f"{mod}.conv1"][0]][0][1], specs[targets[f"{mod}.conv1"][0]][0][0]
            assert (f"{mod}.conv_shortcut" in targets) == (cin != cout), mod
        else:
            assert mod in targets and specs[targets[mod][0]][0][2] == 3, mod
    for mod in ("time_embedding.linear_1", "time_embedding.linear_2", "conv_out"):
        assert mod in targets
    # ... and nothing but norms and biases is left out: every used weight matrix of the model is some module's target
    matrices = {n for n, (s, used) in specs.items() if used and len(s) >= 2}
    assert seen == matrices, sorted(matrices - seen)[:5]
    # self-attention's q / k / v are row blocks of the stacked in_proj, in the import's concatenation order
    for mod in attention_modules(tsd_mod):
        t = mod + ".transformer_blocks.0.attn1."
        pname, r0, rows = targets[t + "to_k"]
        C = specs[pname][0][1]
        assert pname.endswith(".layer4.in_proj.weight") and specs[pname][0] == (3 * C, C) and (r0, rows) == (C, C)
        assert targets[t + "to_q"] == (pname, 0, C) and targets[t + "to_v"] == (pname, 2 * C, C)
        assert targets[mod + ".transformer_blocks.0.attn2.to_k"][0] == pname.replace("layer4.in_proj", "layer6.k_proj")
        assert targets[mod + ".transformer_blocks.0.ff.net.0.proj"] == (pname.replace("layer4.in_proj", "layer8"), 0, 8 * C)
        assert targets[mod + ".proj_out"] == (pname.replace("layer4.in_proj.weight", "layer10.kernel"), 0, C)
    # the columns of every pair a trainer writes fit: cols = prod(shape[1:])
    pairs = _some_pairs(tsd_mod)
    for mod, (down, up) in pairs.items():
        pname, _, rows = targets[mod]
        assert int(np.prod(down.shape[1:])) == int(np.prod(specs[pname][0][1:])) and up.shape[0] == rows


def test_the_12_clip_layers_map_to_rows_of_one_parameter(tsd_mod):
    specs = {n: (s, used) for n, s, used, _ in tsd_mod.param_specs("clip_torch")}
    targets = tsd_mod.lora_targets("clip_torch")
    assert len(targets) == 12 * 6 and targets == tsd_mod.lora_targets("clip")
    for i in range(12):
        h, n = f"text_model.encoder.layers.{i}.", f"player{i + 1}"
        for j, x in enumerate("qkv"):
            assert targets[h + f"self_attn.{x}_proj"] == (n + ".layer2.in_proj.weight", 768 * j, 768)
        assert targets[h + "self_attn.out_proj"] == (n + ".layer2.out_proj.weight", 0, 768)
        assert targets[h + "mlp.fc1"] == (n + ".layer4.weight", 0, 3072) and targets[h + "mlp.fc2"] == (n + ".layer5.weight", 0, 768)
    for mod, (pname, row0, rows) in targets.items():
        shape, used = specs[pname]
        assert used and len(shape) == 2 and row0 + rows <= shape[0] and shape[1] in (768, 3072), (mod, pname)
    with pytest.raises(ValueError):
        tsd_mod.lora_targets("decoder")


class _Recorder:
    """Stands in for a Model: `load_lora` must validate every pair before its first `lora_add`."""

    def __init__(self, tsd_mod, kind):
        self.kind, self.specs, self.calls = tsd_mod.model.KINDS[kind], tsd_mod.param_specs(kind), []

    def param_index(self, name):
        return [s[0] for s in self.specs].index(name)

    def lora_add(self, name, up, down, scale, row0=0):
        self.calls.append((name, up.shape, down.shape, scale, row0))


def test_unknown_keys_and_wrong_shapes_raise_with_nothing_applied(tsd_mod):
    pairs = _some_pairs(tsd_mod)
    good = as_state(pairs, "kohya", alpha=2.0)
    rec = _Recorder(tsd_mod, "diffusion_sd15_torch")
    res = tsd_mod.load_lora(good, unet=rec, scale=0.5)
    assert res == {"applied": len(pairs), "skipped": []} and len(rec.calls) == len(pairs)
    by = {c[0]: c for c in rec.calls}
    name, ushape, dshape, s, row0 = by["unet.layer45.layer4.in_proj.weight"]   # up_blocks.3.attentions.2 attn1.to_k
    assert (ushape, dshape, s, row0) == ((320, 4), (4, 320), 0.5 * 2.0 / 4, 320)
    assert by["unet.layer23.layer2.kernel"][1:3] == ((1280, 4), (4, 2560 * 9))       # conv pair flattened to [O][r] / [r][I * k * k]
    for bad_key in ("lora_unet_down_blocks_9_attentions_0_proj_in.lora_down.weight", "unet.conv_in.weight", "lora_unet_conv_in.lora_sideways.weight",
                    "vae.decoder.conv_in.lora_A.weight", "unet.down_blocks.0.attentions.0.norm.lora_A.weight"):
        rec = _Recorder(tsd_mod, "diffusion_sd15_torch")
        with pytest.raises(ValueError):
            tsd_mod.load_lora(dict(good, **{bad_key: np.zeros((4, 4), np.float32)}), unet=rec)
        assert rec.calls == [], bad_key
    stem = "lora_unet_" + UNDERSCORED.replace(".", "_")
    for key, arr in ((stem + ".lora_down.weight", np.zeros((4, 641), np.float32)), (stem + ".lora_up.weight", np.zeros((639, 4), np.float32)),
                     (stem + ".lora_up.weight", np.zeros((640, 3), np.float32)), ("lora_unet_conv_in.lora_down.weight", np.zeros((4, 4, 1, 1), np.float32))):
        rec = _Recorder(tsd_mod, "diffusion_sd15_torch")
        with pytest.raises(ValueError):
            tsd_mod.load_lora(dict(good, **{key: arr}), unet=rec)
        assert rec.calls == [], key
    lone = {k: v for k, v in good.items() if k != stem + ".lora_up.weight"}
    with pytest.raises(ValueError):
        tsd_mod.load_lora(lone, unet=_Recorder(tsd_mod, "diffusion_sd15_torch"))
    # pairs of a model that was not given are listed, not applied
    te = as_state({"text_model.encoder.layers.0.mlp.fc2": (np.zeros((2, 3072), np.float32), np.zeros((768, 2), np.float32))}, "kohya", None, "text_encoder")
    rec = _Recorder(tsd_mod, "diffusion_sd15_torch")
    res = tsd_mod.load_lora(dict(good, **te), unet=rec)
    assert res == {"applied": len(pairs), "skipped": ["text_encoder.text_model.encoder.layers.0.mlp.fc2"]}
    assert tsd_mod.load_lora(good)["applied"] == 0 and len(tsd_mod.load_lora(good)["skipped"]) == len(pairs)


def test_reference_rounds_once_and_the_interval_holds_for_fp32_sums(tsd_mod):
    """What the GPU tests assume about their own reference: on the exact operands fp32 and float64 agree and fp16 ties occur (so
    nearest-even is exercised); on general operands an fp32 sum in either order stays inside the interval, while a merge from
    fp16-rounded operands leaves it."""
    W, up, down = exact_operands(80, 96, 80, 33, seed=3)
    for s in (0.75, -1.0, 2.0):
        E = tsd_mod.merge_reference(W, up, down, s)
        f32 = W + np.float32(s) * (up @ down)
        assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), E)
    E = tsd_mod.merge_reference(W, up, down, 0.75)
    h = np.float16(E)
    ties = np.abs(E - h.astype(np.float64)) == (np.abs(np.nextafter(h, np.float16(np.inf)).astype(np.float64) - h.astype(np.float64)) / 2)
    assert ties.sum() > 100, int(ties.sum())
    assert np.array_equal(h[ties].view(np.uint16) & 1, np.zeros(int(ties.sum()), np.uint16))   # numpy rounds ties to even
    for O, I, r, s in ((64, 320, 128, 1.0), (40, 77, 5, -0.37), (16, 36, 1, 8.0)):
        W, up, down = general_operands(O, I, O, r, seed=O)
        E, g = tsd_mod.merge_reference(W, up, down, s), gamma(W, up, down, s)
        seq = np.zeros((O, I), np.float32)
        for j in range(r):
            seq += up[:, j:j + 1] * down[j:j + 1, :]
        for what, delta in (("numpy fp32 matmul", up @ down), ("sequential fp32 chain", seq)):
            check_interval(np.float16(W + np.float32(s) * delta), E, g, f"{what} {O}x{I} r={r}")
        rounded = np.float16(W + np.float32(s) * (up.astype(np.float16).astype(np.float32) @ down.astype(np.float16).astype(np.float32)))
        out = (rounded < np.float16(E - g)) | (rounded > np.float16(E + g))
        assert out.mean() > 0.05, out.mean()
