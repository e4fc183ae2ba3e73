"""LoRA adapters for the imported SD-1.x models (extension; no reference counterpart - the reference can only random-initialise).

A model keeps only its packed fp16 weights, so an adapter is merged on the device, in place in the GEMM kernels' own layouts
(`tsd_model_lora_add`, csrc/kernels_lora.hip): W <- rn16(W + s * up @ down), fp32 product on the exact-fp32 matrix instruction, one
rounding to fp16.  The base bits are kept on the device, so `Model.lora_clear()` removes every adapter exactly and another one can
go in without reloading the checkpoint.  Adapters applied one after the other to the same weight stack with one rounding each.

    read_lora(path_or_state)  -> [(module, down, up, alpha)]      kohya and PEFT / diffusers key dialects
    lora_targets(kind)        -> {module: (our parameter, row0, rows)}
    load_lora(path_or_state, unet=..., clip=..., scale=1.0)       s = scale * alpha / rank per pair
    merge_reference(W16, up, down, s)                             the merge in float64 (host twin of the kernel, for tests)

Modules are diffusers paths with the model they belong to in front: "unet.down_blocks.1.attentions.0.proj_in",
"text_encoder.text_model.encoder.layers.3.mlp.fc1".  Pure host code apart from the `lora_add` calls of `load_lora`."""
import numpy as np

from .checkpoint import _ATTN, _RES, _RES_SKIP, _T, _TOP, SD15_MODULES, _layer_kinds, read_safetensors
from .model import KINDS, param_specs

_UNET_KINDS = ("diffusion_sd15_torch", "diffusion_sd15")
_CLIP_KINDS = ("clip_torch", "clip")
_CLIP_LAYER = (("layer2.out_proj", "self_attn.out_proj"), ("layer4", "mlp.fc1"), ("layer5", "mlp.fc2"))  # as hf_clip_text_to_params


def _kind_name(kind):
    if isinstance(kind, str):
        return kind
    for name, k in KINDS.items():
        if k == kind:
            return name
    raise KeyError(f"unknown model kind {kind}")


_TARGETS = {}


def lora_targets(kind):
    """{diffusers module path: (our parameter name, row0, rows)} for every weight matrix of model `kind` that the forward reads and
    an adapter can address: "diffusion_sd15_torch" / "diffusion_sd15" (UNet2DConditionModel paths) or "clip_torch" / "clip"
    (CLIPTextModel paths, with the `text_model.` prefix).  The separate q / k / v projections of self-attention are row blocks of
    the stacked in_proj, in the order the checkpoint import concatenates them.  No GPU needed."""
    kind = _kind_name(kind)
    if kind in _TARGETS:
        return dict(_TARGETS[kind])
    specs = {name: (shape, used) for name, shape, used, _ in param_specs(kind)}
    out = {}

    def put(module, pname, row0=0, rows=None):
        shape, used = specs[pname]
        if used and len(shape) >= 2:  # weight matrices only: no norm weight, no bias, nothing the forward never reads
            out[module] = (pname, row0, shape[0] if rows is None else rows)

    if kind in _UNET_KINDS:
        for ours, theirs in _TOP:
            if theirs.endswith(".weight"):
                put(theirs[:-7], ours)
        kinds = _layer_kinds()
        for i, mod in enumerate(SD15_MODULES, start=1):
            n = f"unet.layer{i}"
            if kinds[i] == "conv":
                put(mod, n + ".kernel")
                continue
            for ours, theirs in (_RES + _RES_SKIP if kinds[i] == "res" else _ATTN):
                if theirs.endswith(".weight"):
                    put(f"{mod}.{theirs[:-7]}", f"{n}.{ours}")
            if kinds[i] == "attn":
                C = specs[n + ".layer4.in_proj.weight"][0][0] // 3
                for j, x in enumerate(("to_q", "to_k", "to_v")):
                    put(f"{mod}.{_T}attn1.{x}", n + ".layer4.in_proj.weight", j * C, C)
    elif kind in _CLIP_KINDS:
        for i in range(12):
            h, n = f"text_model.encoder.layers.{i}.", f"player{i + 1}"
            D = specs[n + ".layer2.in_proj.weight"][0][0] // 3
            for j, x in enumerate("qkv"):
                put(h + f"self_attn.{x}_proj", n + ".layer2.in_proj.weight", j * D, D)
            for ours, theirs in _CLIP_LAYER:
                put(h + theirs, f"{n}.{ours}.weight")
    else:
        raise ValueError(f"no LoRA key map for model kind {kind}")
    _TARGETS[kind] = out
    return dict(out)


_KOHYA = None


def _kohya_table():
    """{"lora_unet_<path with _>": "unet.<path>", "lora_te_...": "text_encoder.<path>"}: the underscore form cannot be split back into
    a path (`to_out_0`, `proj_in`, `down_blocks`), so it is looked up whole."""
    global _KOHYA
    if _KOHYA is None:
        t = {}
        for mod in lora_targets("diffusion_sd15_torch"):
            t["lora_unet_" + mod.replace(".", "_")] = "unet." + mod
        for mod in lora_targets("clip_torch"):
            t["lora_te_" + mod.replace(".", "_")] = "text_encoder." + mod
        _KOHYA = t
    return _KOHYA


_SUFFIX = ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".lora_A.weight", "down"), (".lora_B.weight", "up"),
           (".lora.down.weight", "down"), (".lora.up.weight", "up"), (".alpha", "alpha"))


def _module_of(stem):
    """Canonical module of a key with its suffix removed; None when it names nothing we know."""
    if stem.startswith("lora_unet_") or stem.startswith("lora_te_"):
        return _kohya_table().get(stem)
    if stem.startswith("unet."):
        return stem if stem[5:] in lora_targets("diffusion_sd15_torch") else None
    if stem.startswith("text_encoder."):
        mod = stem[13:]
        if not mod.startswith("text_model."):
            mod = "text_model." + mod
        return "text_encoder." + mod if mod in lora_targets("clip_torch") else None
    return None


def read_lora(path_or_state):
    """[(module, down, up, alpha)] sorted by module, from a safetensors file or a {key: array} state.  down (rank, I) or (rank, I, k, k),
    up (O, rank) or (O, rank, 1, 1), fp32; alpha is a float, or None when the file has none (it then defaults to the rank).
    Dialects: kohya `lora_unet_<path_with_underscores>.lora_down.weight / .lora_up.weight / .alpha` (`lora_te_` for the text
    encoder); PEFT `unet.<path>.lora_A.weight / .lora_B.weight`; diffusers `unet.<path>.lora.down.weight / .lora.up.weight`
    (`text_encoder.` for CLIP, `.alpha` accepted).  A key that is none of these, or a module without both matrices, raises ValueError."""
    state = read_safetensors(path_or_state) if isinstance(path_or_state, str) else path_or_state
    found = {}
    for key in state:
        for suffix, what in _SUFFIX:
            if key.endswith(suffix):
                module = _module_of(key[:-len(suffix)])
                if module is None:
                    raise ValueError(f"LoRA key {key}: no such module in the SD-1.x UNet / text encoder")
                entry = found.setdefault(module, {})
                if what in entry:
                    raise ValueError(f"LoRA key {key}: {module} has a second '{what}' tensor")
                a = np.asarray(state[key], dtype=np.float32)
                entry[what] = float(a.reshape(-1)[0]) if what == "alpha" else a
                break
        else:
            raise ValueError(f"unrecognised LoRA key {key}")
    out = []
    for module in sorted(found):
        e = found[module]
        if "down" not in e or "up" not in e:
            raise ValueError(f"{module}: needs both the down and the up matrix")
        out.append((module, e["down"], e["up"], e.get("alpha")))
    return out


def load_lora(path_or_state, unet=None, clip=None, scale=1.0):
    """Merge every (down, up) pair of the file into `unet` / `clip` (tsd.Diffusion / tsd.CLIP or their Model; kinds
    "diffusion_sd15_torch" and "clip_torch") with s = scale * alpha / rank, alpha defaulting to the rank.
    Returns {"applied": n, "skipped": [modules whose model was not given]}.  Every key and shape is checked before the first merge:
    an unrecognised key or a shape that does not fit its target raises ValueError with nothing applied."""
    pairs = read_lora(path_or_state)
    models = {"unet": getattr(unet, "model", unet), "text_encoder": getattr(clip, "model", clip)}
    plan, skipped = [], []
    for module, down, up, alpha in pairs:
        which, path = module.split(".", 1)
        m = models[which]
        if m is None:
            skipped.append(module)
            continue
        pname, row0, rows = lora_targets(m.kind)[path]
        shape = m.specs[m.param_index(pname)][1]
        cols = int(np.prod(shape[1:]))
        if down.ndim < 2 or up.ndim < 2 or up.shape[1] != down.shape[0] or any(s != 1 for s in up.shape[2:]):
            raise ValueError(f"{module}: down {down.shape} / up {up.shape} are not a low-rank pair")
        rank = down.shape[0]
        if up.shape[0] != rows or int(np.prod(down.shape[1:])) != cols:
            raise ValueError(f"{module}: up {up.shape} / down {down.shape} do not fit {pname} rows [{row0}, {row0 + rows}) x {cols} columns")
        s = float(scale) * (rank if alpha is None else alpha) / rank
        plan.append((m, pname, up.reshape(rows, rank), down.reshape(rank, cols), s, row0))
    for m, pname, u, d, s, row0 in plan:
        m.lora_add(pname, u, d, s, row0=row0)
    return {"applied": len(plan), "skipped": skipped}


def merge_reference(W16, up, down, s):
    """The merge in float64, before the rounding: E = W + s * (up @ down) with W the fp16 weights (any shape with rows first; flattened
    like `down`).  np.float16(E) is the exactly rounded result; the device may differ from it only where its fp32 accumulation does."""
    W = np.asarray(W16, dtype=np.float64)
    u = np.asarray(up, dtype=np.float64).reshape(np.shape(up)[0], -1)
    d = np.asarray(down, dtype=np.float64).reshape(np.shape(down)[0], -1)
    return W + float(s) * (u @ d).reshape(W.shape)
