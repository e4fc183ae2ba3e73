"""Real-checkpoint import for the full-size UNet (extension; no reference counterpart - the
reference can only random-initialise).

A diffusers-layout SD-1.x UNet (`unet/diffusion_pytorch_model.safetensors`: UNet2DConditionModel with block_out_channels
(320, 640, 1280, 1280), 2 resnets per down block, 8 heads, cross_attention_dim 768) maps one-to-one onto model kind
"diffusion_sd15_torch": the 45 flat layers of `SD15_STEPS`, the reference's struct-field names, plus the per-channel norm
parameters.  Pure host code: safetensors is parsed here (8-byte little-endian header length, JSON header, raw
little-endian tensors; F32 / F16 / BF16), the tensors go through `tsd_model_set_param`.

Numerics: fp16 storage of weights and activations with fp32 accumulation; the torch UNet kind uses torch's exact GELU
in the GEGLU gate and per-channel affine norms with eps inside the root, like diffusers."""
import json
import struct

import numpy as np

# flat layer (1-based position in SD15_STEPS) -> diffusers module prefix
SD15_MODULES = (
    ["conv_in"]
    + [f"down_blocks.0.{m}" for m in ("resnets.0", "attentions.0", "resnets.1", "attentions.1", "downsamplers.0.conv")]
    + [f"down_blocks.1.{m}" for m in ("resnets.0", "attentions.0", "resnets.1", "attentions.1", "downsamplers.0.conv")]
    + [f"down_blocks.2.{m}" for m in ("resnets.0", "attentions.0", "resnets.1", "attentions.1", "downsamplers.0.conv")]
    + ["down_blocks.3.resnets.0", "down_blocks.3.resnets.1"]
    + ["mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"]
    + [f"up_blocks.0.{m}" for m in ("resnets.0", "resnets.1", "resnets.2", "upsamplers.0.conv")]
    + [f"up_blocks.1.{m}" for m in ("resnets.0", "attentions.0", "resnets.1", "attentions.1", "resnets.2", "attentions.2",
                                    "upsamplers.0.conv")]
    + [f"up_blocks.2.{m}" for m in ("resnets.0", "attentions.0", "resnets.1", "attentions.1", "resnets.2", "attentions.2",
                                    "upsamplers.0.conv")]
    + [f"up_blocks.3.{m}" for m in ("resnets.0", "attentions.0", "resnets.1", "attentions.1", "resnets.2", "attentions.2")]
)
assert len(SD15_MODULES) == 45

# (our field suffix, diffusers suffix) inside one block; conv weights are `.kernel` on our side
_RES = [("layer1.weight", "norm1.weight"), ("layer1.bias", "norm1.bias"),
        ("layer2.kernel", "conv1.weight"), ("layer2.bias", "conv1.bias"),
        ("layer3.weight", "time_emb_proj.weight"), ("layer3.bias", "time_emb_proj.bias"),
        ("layer4.weight", "norm2.weight"), ("layer4.bias", "norm2.bias"),
        ("layer5.kernel", "conv2.weight"), ("layer5.bias", "conv2.bias")]
_RES_SKIP = [("layer6.kernel", "conv_shortcut.weight"), ("layer6.bias", "conv_shortcut.bias")]
_T = "transformer_blocks.0."
_ATTN = [("layer1.weight", "norm.weight"), ("layer1.bias", "norm.bias"),
         ("layer2.kernel", "proj_in.weight"), ("layer2.bias", "proj_in.bias"),
         ("layer3.weight", _T + "norm1.weight"), ("layer3.bias", _T + "norm1.bias"),
         ("layer4.out_proj.weight", _T + "attn1.to_out.0.weight"), ("layer4.out_proj.bias", _T + "attn1.to_out.0.bias"),
         ("layer5.weight", _T + "norm2.weight"), ("layer5.bias", _T + "norm2.bias"),
         ("layer6.q_proj.weight", _T + "attn2.to_q.weight"), ("layer6.k_proj.weight", _T + "attn2.to_k.weight"),
         ("layer6.v_proj.weight", _T + "attn2.to_v.weight"),
         ("layer6.out_proj.weight", _T + "attn2.to_out.0.weight"), ("layer6.out_proj.bias", _T + "attn2.to_out.0.bias"),
         ("layer7.weight", _T + "norm3.weight"), ("layer7.bias", _T + "norm3.bias"),
         ("layer8.weight", _T + "ff.net.0.proj.weight"), ("layer8.bias", _T + "ff.net.0.proj.bias"),
         ("layer9.weight", _T + "ff.net.2.weight"), ("layer9.bias", _T + "ff.net.2.bias"),
         ("layer10.kernel", "proj_out.weight"), ("layer10.bias", "proj_out.bias")]
_TOP = [("time_embed.layer1.weight", "time_embedding.linear_1.weight"), ("time_embed.layer1.bias", "time_embedding.linear_1.bias"),
        ("time_embed.layer2.weight", "time_embedding.linear_2.weight"), ("time_embed.layer2.bias", "time_embedding.linear_2.bias"),
        ("final.layer1.weight", "conv_norm_out.weight"), ("final.layer1.bias", "conv_norm_out.bias"),
        ("final.layer2.kernel", "conv_out.weight"), ("final.layer2.bias", "conv_out.bias")]

_DT = {"F32": (np.float32, 4), "F16": (np.float16, 2), "BF16": (np.uint16, 2), "F64": (np.float64, 8)}


def read_safetensors(path):
    """{name: float32 array} of every F32 / F16 / BF16 / F64 tensor in the file."""
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        header = json.loads(f.read(n).decode("utf-8"))
        data = f.read()
    out = {}
    for name, meta in header.items():
        if name == "__metadata__":
            continue
        if meta["dtype"] not in _DT:
            raise ValueError(f"{name}: unsupported safetensors dtype {meta['dtype']}")
        dt, size = _DT[meta["dtype"]]
        lo, hi = meta["data_offsets"]
        count = int(np.prod(meta["shape"])) if meta["shape"] else 1
        if hi - lo != count * size:
            raise ValueError(f"{name}: {hi - lo} bytes for shape {meta['shape']} {meta['dtype']}")
        raw = np.frombuffer(data, dtype=dt, count=count, offset=lo)
        if meta["dtype"] == "BF16":
            raw = (raw.astype(np.uint32) << 16).view(np.float32)
        out[name] = np.ascontiguousarray(raw, dtype=np.float32).reshape(meta["shape"])
    return out


def write_safetensors(path, tensors, dtype="F32"):
    """Write {name: array} (tools and tests; F32, F16 or BF16 with round-to-nearest-even)."""
    header, blobs, off = {}, [], 0
    for name in sorted(tensors):
        a = np.ascontiguousarray(tensors[name], dtype=np.float32)
        if dtype == "F32":
            b = a.tobytes()
        elif dtype == "F16":
            b = a.astype(np.float16).tobytes()
        elif dtype == "BF16":
            u = a.view(np.uint32)
            b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).tobytes()
        else:
            raise ValueError(dtype)
        header[name] = {"dtype": dtype, "shape": list(a.shape), "data_offsets": [off, off + len(b)]}
        blobs.append(b)
        off += len(b)
    h = json.dumps(header, separators=(",", ":")).encode("utf-8")
    h += b" " * ((8 - len(h) % 8) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)))
        f.write(h)
        for b in blobs:
            f.write(b)


def _layer_kinds():
    """{flat layer position: "conv" | "res" | "attn"} from the library's own parameter inventory."""
    from .model import param_specs
    fields = {}
    for name, _, _, _ in param_specs("diffusion_sd15"):
        if name.startswith("unet.layer"):
            fields.setdefault(int(name.split(".")[1][5:]), set()).add(name.split(".", 2)[2])
    return {i: ("attn" if "layer4.in_proj.weight" in f else "res" if "layer3.weight" in f else "conv")
            for i, f in fields.items()}


def _layers_from_diffusers(state, prefix, modules, out):
    """The flat layers `unet.layer1 ..` of `modules` (a prefix of SD15_MODULES) from a diffusers state dict into `out`."""
    g = lambda k: np.asarray(state[prefix + k], dtype=np.float32)  # noqa: E731
    kinds = _layer_kinds()
    for i, mod in enumerate(modules, start=1):
        n, kind = f"unet.layer{i}", kinds[i]
        if kind == "conv":
            out[n + ".kernel"], out[n + ".bias"] = g(mod + ".weight"), g(mod + ".bias")
        elif kind == "res":
            for ours, theirs in _RES:
                out[f"{n}.{ours}"] = g(f"{mod}.{theirs}")
            if prefix + f"{mod}.conv_shortcut.weight" in state:
                for ours, theirs in _RES_SKIP:
                    out[f"{n}.{ours}"] = g(f"{mod}.{theirs}")
        else:
            for ours, theirs in _ATTN:
                a = g(f"{mod}.{theirs}")
                if ours.endswith(".kernel") and a.ndim == 2:  # SD-2.x style linear projection
                    a = a[:, :, None, None]
                out[f"{n}.{ours}"] = a
            t = f"{mod}.{_T}attn1."
            out[n + ".layer4.in_proj.weight"] = np.concatenate([g(t + "to_q.weight"), g(t + "to_k.weight"), g(t + "to_v.weight")])
    return out


def _layers_to_diffusers(params, prefix, modules, out):
    """Inverse of `_layers_from_diffusers`."""
    kinds = _layer_kinds()
    for i, mod in enumerate(modules, start=1):
        n, kind = f"unet.layer{i}", kinds[i]
        if kind == "conv":
            out[prefix + mod + ".weight"], out[prefix + mod + ".bias"] = params[n + ".kernel"], params[n + ".bias"]
        elif kind == "res":
            for ours, theirs in _RES:
                out[prefix + f"{mod}.{theirs}"] = params[f"{n}.{ours}"]
            w = params.get(n + ".layer6.kernel")
            if w is not None and w.shape[0] != w.shape[1]:
                for ours, theirs in _RES_SKIP:
                    out[prefix + f"{mod}.{theirs}"] = params[f"{n}.{ours}"]
        else:
            for ours, theirs in _ATTN:
                out[prefix + f"{mod}.{theirs}"] = params[f"{n}.{ours}"]
            q, k, v = np.split(np.asarray(params[n + ".layer4.in_proj.weight"]), 3)
            t = prefix + f"{mod}.{_T}attn1."
            out[t + "to_q.weight"], out[t + "to_k.weight"], out[t + "to_v.weight"] = q, k, v
    return out


def diffusers_sd15_unet_to_params(state, prefix=""):
    """diffusers UNet2DConditionModel state dict -> {our parameter name: array} for kind "diffusion_sd15_torch"."""
    g = lambda k: np.asarray(state[prefix + k], dtype=np.float32)  # noqa: E731
    return _layers_from_diffusers(state, prefix, SD15_MODULES, {ours: g(theirs) for ours, theirs in _TOP})


def params_to_diffusers_sd15_unet(params, prefix=""):
    """Inverse of `diffusers_sd15_unet_to_params` (export; used by the round-trip test)."""
    return _layers_to_diffusers(params, prefix, SD15_MODULES, {prefix + theirs: np.asarray(params[ours], np.float32) for ours, theirs in _TOP})


def load_sd15_unet(path, ctx=None, prefix=""):
    """tsd.Diffusion(variant="diffusion_sd15_torch") with the weights of a diffusers SD-1.x UNet safetensors file."""
    from .diffusion import Diffusion
    from .model import param_specs
    params = diffusers_sd15_unet_to_params(read_safetensors(path), prefix)
    for name, shape, used, _ in param_specs("diffusion_sd15_torch"):
        if name not in params:
            if used:
                raise KeyError(f"checkpoint has no tensor for {name}")
            params[name] = np.zeros(shape, np.float32)  # fields the reference allocates but never reads
        elif tuple(params[name].shape) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {params[name].shape}, model expects {shape}")
    return Diffusion(ctx=ctx, params=params, variant="diffusion_sd15_torch")


# ---- SD-2.x UNet (diffusers UNet2DConditionModel with attention_head_dim (5, 10, 20, 20), cross_attention_dim 1024 and
# use_linear_projection -> model kind "diffusion_sd2") ----
# The modules and the tensor names are SD-1.x's.  use_linear_projection only changes the rank of proj_in / proj_out in the file ([C, C]
# instead of [C, C, 1, 1]); the head split lives in the model kind, not in any tensor's shape.
def diffusers_sd2_unet_to_params(state, prefix=""):
    """diffusers SD-2.x UNet state dict -> {our parameter name: array} for kind "diffusion_sd2"; proj_in / proj_out 2-D or 4-D."""
    return diffusers_sd15_unet_to_params(state, prefix)


def params_to_diffusers_sd2_unet(params, prefix="", linear_projection=True):
    """Inverse of `diffusers_sd2_unet_to_params`; linear_projection: proj_in / proj_out as [C, C] (how the SD-2.x files hold them)."""
    out = params_to_diffusers_sd15_unet(params, prefix)
    if linear_projection:
        for k in list(out):
            if k.endswith(("proj_in.weight", "proj_out.weight")) and np.ndim(out[k]) == 4:
                out[k] = np.asarray(out[k])[:, :, 0, 0]
    return out


def load_sd2_unet(path_or_state, ctx=None, prefix=""):
    """tsd.Diffusion(variant="diffusion_sd2") with the weights of a diffusers SD-2.x UNet: a safetensors file, or its state dict."""
    from .diffusion import Diffusion
    from .model import param_specs
    state = read_safetensors(path_or_state) if isinstance(path_or_state, str) else path_or_state
    params = diffusers_sd2_unet_to_params(state, prefix)
    for name, shape, used, _ in param_specs("diffusion_sd2"):
        if name not in params:
            if used:
                raise KeyError(f"checkpoint has no tensor for {name}")
            params[name] = np.zeros(shape, np.float32)
        elif tuple(params[name].shape) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {params[name].shape}, model expects {shape}")
    return Diffusion(ctx=ctx, params=params, variant="diffusion_sd2")


# ---- ControlNet (diffusers `ControlNetModel` for SD-1.x -> model kind "controlnet_sd15_torch") ------------------------------------------
# the UNet's encoder and bottleneck under the UNet's own names (the first 21 flat layers), the hint encoder and the zero convolutions
CONTROLNET_LAYERS = 21
CONTROLNET_MODULES = SD15_MODULES[:CONTROLNET_LAYERS]
CONTROLNET_HINT_MODULES = (["controlnet_cond_embedding.conv_in"] + [f"controlnet_cond_embedding.blocks.{i}" for i in range(6)]
                           + ["controlnet_cond_embedding.conv_out"])
_CN_CONVS = ([(f"hint.conv{i}", m) for i, m in enumerate(CONTROLNET_HINT_MODULES, start=1)]
             + [(f"zero.skip{i + 1}", f"controlnet_down_blocks.{i}") for i in range(12)] + [("zero.mid", "controlnet_mid_block")])
_CN_TOP = _TOP[:4]   # the time embedding; a ControlNet has no output layer


def diffusers_controlnet_to_params(state, prefix=""):
    """diffusers ControlNetModel state dict -> {our parameter name: array} for kind "controlnet_sd15_torch"."""
    g = lambda k: np.asarray(state[prefix + k], dtype=np.float32)  # noqa: E731
    out = {ours: g(theirs) for ours, theirs in _CN_TOP}
    for ours, theirs in _CN_CONVS:
        out[ours + ".kernel"], out[ours + ".bias"] = g(theirs + ".weight"), g(theirs + ".bias")
    return _layers_from_diffusers(state, prefix, CONTROLNET_MODULES, out)


def params_to_diffusers_controlnet(params, prefix=""):
    """Inverse of `diffusers_controlnet_to_params` (export; used by the round-trip test)."""
    out = {prefix + theirs: np.asarray(params[ours], np.float32) for ours, theirs in _CN_TOP}
    for ours, theirs in _CN_CONVS:
        out[prefix + theirs + ".weight"], out[prefix + theirs + ".bias"] = params[ours + ".kernel"], params[ours + ".bias"]
    return _layers_to_diffusers(params, prefix, CONTROLNET_MODULES, out)


def controlnet_params_complete(params):
    """`params` with zeros for the fields the reference's structs allocate but never read; KeyError / ValueError for a missing or misshapen
    tensor that the forward does read."""
    from .model import param_specs
    params = dict(params)
    for name, shape, used, _ in param_specs("controlnet_sd15_torch"):
        if name not in params:
            if used:
                raise KeyError(f"checkpoint has no tensor for {name}")
            params[name] = np.zeros(shape, np.float32)
        elif tuple(np.shape(params[name])) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {np.shape(params[name])}, model expects {shape}")
    return params


def load_controlnet(path_or_state, ctx=None, prefix=""):
    """tsd.ControlNet(variant="controlnet_sd15_torch") with the weights of a diffusers SD-1.x ControlNetModel: a safetensors file, or its
    state dict."""
    from .diffusion import ControlNet
    state = read_safetensors(path_or_state) if isinstance(path_or_state, str) else path_or_state
    return ControlNet(ctx=ctx, params=controlnet_params_complete(diffusers_controlnet_to_params(state, prefix)), variant="controlnet_sd15_torch")


# ---- IP-Adapter (the published ip-adapter_sd15 safetensors -> model kind "ip_adapter_sd15") ------------------------------------------------
# widths of the 16 cross-attention blocks in the published files' order: `ip_adapter.{1, 3, .., 31}`
IP_ADAPTER_PUBLISHED_WIDTHS = (320, 320, 640, 640, 1280, 1280) + (1280,) * 3 + (640,) * 3 + (320,) * 3 + (1280,)


def ip_adapter_to_params(state, prefix=""):
    """Published IP-Adapter state dict -> {our parameter name: array} for kind "ip_adapter_sd15".

    THE KEY MAP (the single place to correct it).  The published file holds `image_proj.proj.{weight,bias}`, `image_proj.norm.{weight,bias}`
    and `ip_adapter.<i>.to_k_ip.weight` / `ip_adapter.<i>.to_v_ip.weight` for i = 1, 3, .., 31.  The odd index 2k + 1 is the k-th
    cross-attention processor in diffusers' module order (every transformer block has a self-attention processor, even index, in front of
    it): the down blocks (k = 0 .. 5, widths 320, 320, 640, 640, 1280, 1280), then the up blocks (k = 6 .. 14, widths 1280 x3, 640 x3,
    320 x3), then the mid block (k = 15, width 1280).  The model keeps these names; only its ORDER differs - the step table's: the six
    encoder blocks (1 .. 11), the bottleneck (31), the nine decoder blocks (13 .. 29).  This order is stated from the layout of diffusers'
    UNet2DConditionModel, not checked against a real file here: a file whose 16 widths do not follow the sequence above is refused
    (ValueError), so a different processor order cannot load silently."""
    g = lambda k: np.asarray(state[prefix + k], dtype=np.float32)  # noqa: E731
    out = {k: g(k) for k in ("image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias")}
    widths = []
    for k in range(16):
        for f in ("to_k_ip", "to_v_ip"):
            name = f"ip_adapter.{2 * k + 1}.{f}.weight"
            if prefix + name not in state:
                raise KeyError(f"checkpoint has no tensor {prefix + name}")
            out[name] = g(name)
        wk, wv = out[f"ip_adapter.{2 * k + 1}.to_k_ip.weight"].shape, out[f"ip_adapter.{2 * k + 1}.to_v_ip.weight"].shape
        if wk != wv or len(wk) != 2:
            raise ValueError(f"ip_adapter.{2 * k + 1}: to_k_ip {wk} and to_v_ip {wv} differ in shape")
        widths.append(int(wk[0]))
    if tuple(widths) != IP_ADAPTER_PUBLISHED_WIDTHS:
        raise ValueError(f"the 16 cross-attention widths of this file are {widths}; the key map assumes {list(IP_ADAPTER_PUBLISHED_WIDTHS)} "
                         "(down blocks, up blocks, mid block): see ip_adapter_to_params")
    return out


def params_to_ip_adapter(params, prefix=""):
    """Inverse of `ip_adapter_to_params` (export; used by the round-trip test): the published key layout, in the published order."""
    names = ["image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias"]
    names += [f"ip_adapter.{2 * k + 1}.{f}.weight" for k in range(16) for f in ("to_k_ip", "to_v_ip")]
    return {prefix + n: np.asarray(params[n], np.float32) for n in names}


def load_ip_adapter(path_or_state, ctx=None, prefix=""):
    """tsd.IPAdapter with the weights of a published SD-1.5 IP-Adapter file (ip-adapter_sd15: 4 image tokens from the 1024-wide CLIP image
    embedding): a safetensors file, or its state dict.  The "plus" files (a resampler instead of image_proj.proj) are another model
    kind: `load_ip_adapter_plus` reads them."""
    from .diffusion import IPAdapter
    from .model import param_specs
    state = read_safetensors(path_or_state) if isinstance(path_or_state, str) else path_or_state
    if prefix + "image_proj.proj.weight" not in state:
        raise KeyError("checkpoint has no image_proj.proj.weight: not an ip-adapter_sd15 file (the 'plus' files carry a resampler: "
                       "load_ip_adapter_plus reads those)")
    params = ip_adapter_to_params(state, prefix)
    for name, shape, _, _ in param_specs("ip_adapter_sd15"):
        if tuple(np.shape(params[name])) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {np.shape(params[name])}, model expects {shape}")
    return IPAdapter(ctx=ctx, params=params)


# ---- IP-Adapter Plus (the published ip-adapter-plus_sd15 / ip-adapter-plus-face_sd15 safetensors -> kind "ip_adapter_plus_sd15") ----------
IP_ADAPTER_PLUS_DEPTH = 4


def ip_adapter_plus_names():
    """The 83 tensor names of a plus file, in the resampler's state-dict order and then the 16 pairs in the PUBLISHED order (1, 3, .., 31)."""
    names = ["image_proj.latents", "image_proj.proj_in.weight", "image_proj.proj_in.bias", "image_proj.proj_out.weight",
             "image_proj.proj_out.bias", "image_proj.norm_out.weight", "image_proj.norm_out.bias"]
    for l in range(IP_ADAPTER_PLUS_DEPTH):
        n = f"image_proj.layers.{l}."
        names += [n + t for t in ("0.norm1.weight", "0.norm1.bias", "0.norm2.weight", "0.norm2.bias", "0.to_q.weight", "0.to_kv.weight",
                                  "0.to_out.weight", "1.0.weight", "1.0.bias", "1.1.weight", "1.3.weight")]
    return names + [f"ip_adapter.{2 * k + 1}.{f}.weight" for k in range(16) for f in ("to_k_ip", "to_v_ip")]


def ip_adapter_plus_to_params(state, prefix=""):
    """Published IP-Adapter Plus state dict -> {our parameter name: array} for kind "ip_adapter_plus_sd15".

    The model keeps the published names, so the map is the identity on 83 tensors; what this function does is refuse.  `image_proj` is
    `Resampler(dim=768, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=768, ff_mult=4)` of the published
    IP-Adapter code: `latents` [1][16][768], `proj_in` 1280 -> 768 and `proj_out` 768 -> 768 with bias, `norm_out`, and per layer L
    `layers.L.0` = PerceiverAttention (norm1 for the image rows, norm2 for the latents, bias-free to_q [768][768], to_kv [1536][768] with
    the K half first, to_out [768][768]) and `layers.L.1` = Sequential(LayerNorm, Linear(768, 3072), GELU, Linear(3072, 768)), both linears
    bias-free, hence the indices 0, 1, 3.  These names, shapes and the module's arithmetic (tests/ipplus_ref.py restates it) are written
    FROM MEMORY of that module, not checked against a real file or the published code here: a file that lacks one of the 83 names is
    refused by name (KeyError), one whose `latents` are not [1][16][768] or whose `proj_in` is not [768][1280] with the shape named
    (ValueError; those are the full-face, SDXL and ViT-L files), and the 16 pairs pass `ip_adapter_to_params`'s width-order check."""
    missing = [n for n in ip_adapter_plus_names() if prefix + n not in state]
    if missing:
        if prefix + "image_proj.latents" not in state and prefix + "image_proj.proj.weight" in state:
            raise KeyError(f"checkpoint has no tensor {prefix}image_proj.latents but an image_proj.proj.weight: an ip-adapter_sd15 file, "
                           "load_ip_adapter reads it")
        raise KeyError(f"checkpoint has no tensor {prefix + missing[0]}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    out = {n: np.asarray(state[prefix + n], dtype=np.float32) for n in ip_adapter_plus_names()}
    if out["image_proj.latents"].shape != (1, 16, 768):
        raise ValueError(f"image_proj.latents has shape {out['image_proj.latents'].shape}, the model expects (1, 16, 768): not an "
                         "ip-adapter-plus_sd15 file (another query count or width: the SDXL and full-face files)")
    if out["image_proj.proj_in.weight"].shape != (768, 1280):
        raise ValueError(f"image_proj.proj_in.weight has shape {out['image_proj.proj_in.weight'].shape}, the model expects (768, 1280): "
                         "the resampler of this file does not read the ViT-H/14 hidden states (the ViT-L and SDXL files)")
    widths = []
    for k in range(16):
        wk, wv = out[f"ip_adapter.{2 * k + 1}.to_k_ip.weight"].shape, out[f"ip_adapter.{2 * k + 1}.to_v_ip.weight"].shape
        if wk != wv or len(wk) != 2:
            raise ValueError(f"ip_adapter.{2 * k + 1}: to_k_ip {wk} and to_v_ip {wv} differ in shape")
        widths.append(int(wk[0]))
    if tuple(widths) != IP_ADAPTER_PUBLISHED_WIDTHS:
        raise ValueError(f"the 16 cross-attention widths of this file are {widths}; the key map assumes {list(IP_ADAPTER_PUBLISHED_WIDTHS)} "
                         "(down blocks, up blocks, mid block): see ip_adapter_to_params")
    return out


def params_to_ip_adapter_plus(params, prefix=""):
    """Inverse of `ip_adapter_plus_to_params` (export; used by the round-trip test): the published names, the pairs in the published order."""
    return {prefix + n: np.asarray(params[n], np.float32) for n in ip_adapter_plus_names()}


def load_ip_adapter_plus(path_or_state, ctx=None, prefix=""):
    """tsd.IPAdapter(variant="ip_adapter_plus_sd15") with the weights of a published SD-1.5 IP-Adapter Plus file (ip-adapter-plus_sd15,
    ip-adapter-plus-face_sd15: 16 image tokens resampled from the ViT-H/14 hidden states): a safetensors file, or its state dict.  The
    layout is stated from memory of the published module, not checked against a real file here (`ip_adapter_plus_to_params`); every
    tensor's shape is checked against the model's inventory before anything is uploaded."""
    from .diffusion import IPAdapter
    from .model import param_specs
    state = read_safetensors(path_or_state) if isinstance(path_or_state, str) else path_or_state
    params = ip_adapter_plus_to_params(state, prefix)
    for name, shape, _, _ in param_specs("ip_adapter_plus_sd15"):
        if tuple(np.shape(params[name])) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {np.shape(params[name])}, model expects {shape}")
    return IPAdapter(ctx=ctx, params=params, variant="ip_adapter_plus_sd15")


# ---- CLIP vision encoder (HF CLIPVisionModelWithProjection, the `image_encoder/` folder of the IP-Adapter files -> kind "clip_vision_h") ----
_CV_LAYER = (("ln1", "layer_norm1"), ("out_proj", "self_attn.out_proj"), ("ln2", "layer_norm2"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"))
CLIP_VISION_WIDTH = 1280


def clip_vision_to_params(state, prefix=""):
    """Hugging Face CLIPVisionModelWithProjection state dict (tensors or arrays) -> {our parameter name: array} for kind "clip_vision_h".

    THE KEY MAP: `vision_model.embeddings.class_embedding` [1280], `.patch_embedding.weight` [1280][3][14][14] (flattened to [1280][588],
    column c * 196 + kh * 14 + kw) and `.position_embedding.weight` [257][1280]; `vision_model.pre_layrnorm` (HF's spelling);
    `vision_model.encoder.layers.N.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.fc1, mlp.fc2}` with q / k / v stacked into
    `layers.N.in_proj`; `vision_model.post_layernorm`; `visual_projection.weight` [1024][1280].  A `position_ids` buffer is ignored.  As
    many layers as the state dict holds are mapped (the model wants 32).  ValueError for a missing tensor, naming it, and for a state
    dict of another width (a ViT-L file is 1024 wide)."""
    def g(k):
        if prefix + k not in state:
            raise ValueError(f"checkpoint has no tensor {prefix + k}")
        v = state[prefix + k]
        return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)

    vm = "vision_model."
    cls = g(vm + "embeddings.class_embedding").reshape(-1)
    if cls.shape[0] != CLIP_VISION_WIDTH:
        raise ValueError(f"this vision tower is {cls.shape[0]} wide; kind clip_vision_h is OpenCLIP ViT-H/14, {CLIP_VISION_WIDTH} wide "
                         "(a ViT-L/14 file is 1024 wide)")
    pw = g(vm + "embeddings.patch_embedding.weight")
    if pw.shape != (CLIP_VISION_WIDTH, 3, 14, 14):
        raise ValueError(f"{prefix + vm}embeddings.patch_embedding.weight has shape {pw.shape}, expected {(CLIP_VISION_WIDTH, 3, 14, 14)}")
    out = {"embeddings.class_embedding": cls, "embeddings.patch_embedding.weight": pw.reshape(CLIP_VISION_WIDTH, 588),
           "embeddings.position_embedding.weight": g(vm + "embeddings.position_embedding.weight")}
    for ours, theirs in (("pre_layrnorm", vm + "pre_layrnorm"), ("post_layernorm", vm + "post_layernorm")):
        out[ours + ".weight"], out[ours + ".bias"] = g(theirs + ".weight"), g(theirs + ".bias")
    i = 0
    while prefix + vm + f"encoder.layers.{i}.layer_norm1.weight" in state:
        h, n = vm + f"encoder.layers.{i}.", f"layers.{i}"
        out[n + ".in_proj.weight"] = np.concatenate([g(h + f"self_attn.{x}_proj.weight") for x in "qkv"])
        out[n + ".in_proj.bias"] = np.concatenate([g(h + f"self_attn.{x}_proj.bias") for x in "qkv"])
        for ours, theirs in _CV_LAYER:
            out[f"{n}.{ours}.weight"], out[f"{n}.{ours}.bias"] = g(h + theirs + ".weight"), g(h + theirs + ".bias")
        i += 1
    out["visual_projection.weight"] = g("visual_projection.weight")
    return out


def params_to_clip_vision(params, prefix=""):
    """Inverse of `clip_vision_to_params` (export; used by the round-trip test): HF's key layout, the patch embedding as a convolution."""
    p = lambda k: np.asarray(params[k], np.float32)  # noqa: E731
    vm = prefix + "vision_model."
    out = {vm + "embeddings.class_embedding": p("embeddings.class_embedding"),
           vm + "embeddings.patch_embedding.weight": p("embeddings.patch_embedding.weight").reshape(-1, 3, 14, 14),
           vm + "embeddings.position_embedding.weight": p("embeddings.position_embedding.weight"),
           prefix + "visual_projection.weight": p("visual_projection.weight")}
    for ours in ("pre_layrnorm", "post_layernorm"):
        out[vm + ours + ".weight"], out[vm + ours + ".bias"] = p(ours + ".weight"), p(ours + ".bias")
    i = 0
    while f"layers.{i}.ln1.weight" in params:
        h, n = vm + f"encoder.layers.{i}.", f"layers.{i}"
        for x, w, b in zip("qkv", np.split(p(n + ".in_proj.weight"), 3), np.split(p(n + ".in_proj.bias"), 3)):
            out[h + f"self_attn.{x}_proj.weight"], out[h + f"self_attn.{x}_proj.bias"] = w, b
        for ours, theirs in _CV_LAYER:
            out[h + theirs + ".weight"], out[h + theirs + ".bias"] = p(f"{n}.{ours}.weight"), p(f"{n}.{ours}.bias")
        i += 1
    return out


def load_clip_vision(path_or_state, ctx=None, prefix=""):
    """tsd.CLIPVision with the weights of a CLIPVisionModelWithProjection safetensors file (`image_encoder/model.safetensors` of
    h94/IP-Adapter: OpenCLIP ViT-H/14) or its state dict.  ValueError for a missing tensor (named), another width, another shape."""
    from .clip import CLIPVision
    from .model import param_specs
    state = read_safetensors(path_or_state) if isinstance(path_or_state, str) else path_or_state
    params = clip_vision_to_params(state, prefix)
    for name, shape, _, _ in param_specs("clip_vision_h"):
        if name not in params:
            raise ValueError(f"checkpoint has no tensor for {name} (the encoder has 32 layers)")
        if tuple(np.shape(params[name])) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {np.shape(params[name])}, model expects {shape}")
    return CLIPVision(ctx=ctx, params=params)


def hf_clip_text_to_params(state):
    """Hugging Face CLIPTextModel state dict (with or without the `text_model.` prefix; tensors or arrays) ->
    {our parameter name: array} for kind "clip_torch" (q/k/v stacked into the reference's in_proj), or for kind "clip_sd2" when the
    state dict is 1024 wide (the SD-2.x text encoder: 23 layers); `clip_text_variant` names the kind."""
    pre = "text_model." if any(k.startswith("text_model.") for k in state) else ""

    def g(k):
        v = state[pre + k]
        return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)

    out = {"embedding.token.weight": g("embeddings.token_embedding.weight"),
           "embedding.position": g("embeddings.position_embedding.weight").reshape(-1),
           "layernorm.weight": g("final_layer_norm.weight"), "layernorm.bias": g("final_layer_norm.bias")}
    for i in range(23 if out["embedding.token.weight"].shape[1] == 1024 else 12):
        h, n = f"encoder.layers.{i}.", f"player{i + 1}"
        out[n + ".layer2.in_proj.weight"] = np.concatenate([g(h + f"self_attn.{x}_proj.weight") for x in "qkv"])
        out[n + ".layer2.in_proj.bias"] = np.concatenate([g(h + f"self_attn.{x}_proj.bias") for x in "qkv"])
        for ours, theirs in (("layer2.out_proj", "self_attn.out_proj"), ("layer4", "mlp.fc1"), ("layer5", "mlp.fc2"),
                             ("layer1", "layer_norm1"), ("layer3", "layer_norm2")):
            out[f"{n}.{ours}.weight"], out[f"{n}.{ours}.bias"] = g(h + theirs + ".weight"), g(h + theirs + ".bias")
    return out


def clip_text_variant(params):
    """"clip_sd2" for the 1024-wide SD-2.x text encoder, else "clip_torch"."""
    return "clip_sd2" if np.shape(params["embedding.token.weight"])[1] == 1024 else "clip_torch"


def params_to_hf_clip_text(params, prefix="text_model."):
    """Inverse of `hf_clip_text_to_params` (export; used by the round-trip test)."""
    p = lambda k: np.asarray(params[k], np.float32)  # noqa: E731
    width = p("embedding.token.weight").shape[1]
    out = {prefix + "embeddings.token_embedding.weight": p("embedding.token.weight"),
           prefix + "embeddings.position_embedding.weight": p("embedding.position").reshape(-1, width),
           prefix + "final_layer_norm.weight": p("layernorm.weight"), prefix + "final_layer_norm.bias": p("layernorm.bias")}
    i = 0
    while f"player{i + 1}.layer4.weight" in params:
        h, n = prefix + f"encoder.layers.{i}.", f"player{i + 1}"
        for x, w, b in zip("qkv", np.split(p(n + ".layer2.in_proj.weight"), 3), np.split(p(n + ".layer2.in_proj.bias"), 3)):
            out[h + f"self_attn.{x}_proj.weight"], out[h + f"self_attn.{x}_proj.bias"] = w, b
        for ours, theirs in (("layer2.out_proj", "self_attn.out_proj"), ("layer4", "mlp.fc1"), ("layer5", "mlp.fc2"),
                             ("layer1", "layer_norm1"), ("layer3", "layer_norm2")):
            out[h + theirs + ".weight"], out[h + theirs + ".bias"] = p(f"{n}.{ours}.weight"), p(f"{n}.{ours}.bias")
        i += 1
    return out


def load_clip_text(path_or_state, ctx=None):
    """tsd.CLIP from a CLIPTextModel safetensors file (e.g. `text_encoder/model.safetensors`) or an in-memory state dict: variant
    "clip_torch" for an SD-1.x repository, "clip_sd2" when the state dict is 1024 wide (SD-2.x)."""
    from .clip import CLIP
    state = read_safetensors(path_or_state) if isinstance(path_or_state, str) else path_or_state
    params = hf_clip_text_to_params(state)
    return CLIP(ctx=ctx, params=params, variant=clip_text_variant(params))


# ---- VAE (diffusers AutoencoderKL) ---------------------------------------------------------------------------------
# layer position in DECODER_LAYERS / ENCODER_LAYERS (1-based) -> diffusers module; None = no parameters
VAE_DECODER_MODULES = {1: "post_quant_conv", 2: "decoder.conv_in", 3: "decoder.mid_block.resnets.0",
                       4: "decoder.mid_block.attentions.0", 5: "decoder.mid_block.resnets.1",
                       6: "decoder.up_blocks.0.resnets.0", 7: "decoder.up_blocks.0.resnets.1", 8: "decoder.up_blocks.0.resnets.2",
                       10: "decoder.up_blocks.0.upsamplers.0.conv",
                       11: "decoder.up_blocks.1.resnets.0", 12: "decoder.up_blocks.1.resnets.1", 13: "decoder.up_blocks.1.resnets.2",
                       15: "decoder.up_blocks.1.upsamplers.0.conv",
                       16: "decoder.up_blocks.2.resnets.0", 17: "decoder.up_blocks.2.resnets.1", 18: "decoder.up_blocks.2.resnets.2",
                       20: "decoder.up_blocks.2.upsamplers.0.conv",
                       21: "decoder.up_blocks.3.resnets.0", 22: "decoder.up_blocks.3.resnets.1", 23: "decoder.up_blocks.3.resnets.2",
                       24: "decoder.conv_norm_out", 26: "decoder.conv_out"}
VAE_ENCODER_MODULES = {1: "encoder.conv_in", 2: "encoder.down_blocks.0.resnets.0", 3: "encoder.down_blocks.0.resnets.1",
                       4: "encoder.down_blocks.0.downsamplers.0.conv",
                       5: "encoder.down_blocks.1.resnets.0", 6: "encoder.down_blocks.1.resnets.1",
                       7: "encoder.down_blocks.1.downsamplers.0.conv",
                       8: "encoder.down_blocks.2.resnets.0", 9: "encoder.down_blocks.2.resnets.1",
                       10: "encoder.down_blocks.2.downsamplers.0.conv",
                       11: "encoder.down_blocks.3.resnets.0", 12: "encoder.down_blocks.3.resnets.1",
                       13: "encoder.mid_block.resnets.0", 14: "encoder.mid_block.attentions.0", 15: "encoder.mid_block.resnets.1",
                       16: "encoder.conv_norm_out", 18: "encoder.conv_out", 19: "quant_conv"}
_VRES = [("group_norm1.weight", "norm1.weight"), ("group_norm1.bias", "norm1.bias"), ("conv1.kernel", "conv1.weight"),
         ("conv1.bias", "conv1.bias"), ("group_norm2.weight", "norm2.weight"), ("group_norm2.bias", "norm2.bias"),
         ("conv2.kernel", "conv2.weight"), ("conv2.bias", "conv2.bias")]
_VRES_SKIP = [("res_conv_layer.kernel", "conv_shortcut.weight"), ("res_conv_layer.bias", "conv_shortcut.bias")]


def _vae_kinds(which):
    from .model import param_specs
    fields = {}
    for name, _, _, _ in param_specs(which + "_torch"):
        i, f = name.split(".", 1)
        fields.setdefault(int(i[1:]), set()).add(f)
    return {i: ("attn" if "attention.in_proj.weight" in f else "res" if "conv1.kernel" in f else
                "conv" if "kernel" in f else "gn") for i, f in fields.items()}


def diffusers_vae_to_params(state, which):
    """diffusers AutoencoderKL state dict -> {our parameter name: array} for kind "decoder_torch" / "encoder_torch".
    Attention projections may be named to_q/to_k/to_v/to_out.0 (current) or query/key/value/proj_attn (older files);
    1x1-conv shaped attention weights (C, C, 1, 1) are flattened."""
    mods = VAE_DECODER_MODULES if which == "decoder" else VAE_ENCODER_MODULES
    g = lambda k: np.asarray(state[k], dtype=np.float32)  # noqa: E731
    out = {}
    for i, kind in _vae_kinds(which).items():
        n, mod = f"l{i}", mods[i]
        if kind == "conv":
            out[n + ".kernel"], out[n + ".bias"] = g(mod + ".weight"), g(mod + ".bias")
        elif kind == "gn":
            out[n + ".weight"], out[n + ".bias"] = g(mod + ".weight"), g(mod + ".bias")
        elif kind == "res":
            for ours, theirs in _VRES:
                out[f"{n}.{ours}"] = g(f"{mod}.{theirs}")
            if f"{mod}.conv_shortcut.weight" in state:
                for ours, theirs in _VRES_SKIP:
                    out[f"{n}.{ours}"] = g(f"{mod}.{theirs}")
        else:
            names = ("to_q", "to_k", "to_v", "to_out.0") if f"{mod}.to_q.weight" in state else ("query", "key", "value", "proj_attn")
            flat = lambda k: g(k).reshape(g(k).shape[0], -1)  # noqa: E731
            out[n + ".attention.in_proj.weight"] = np.concatenate([flat(f"{mod}.{x}.weight") for x in names[:3]])
            out[n + ".attention.in_proj.bias"] = np.concatenate([g(f"{mod}.{x}.bias") for x in names[:3]])
            out[n + ".attention.out_proj.weight"], out[n + ".attention.out_proj.bias"] = flat(f"{mod}.{names[3]}.weight"), g(f"{mod}.{names[3]}.bias")
            out[n + ".group_norm.weight"], out[n + ".group_norm.bias"] = g(mod + ".group_norm.weight"), g(mod + ".group_norm.bias")
    return out


def params_to_diffusers_vae(params, which):
    """Inverse of `diffusers_vae_to_params` (current diffusers attention names)."""
    mods = VAE_DECODER_MODULES if which == "decoder" else VAE_ENCODER_MODULES
    out = {}
    for i, kind in _vae_kinds(which).items():
        n, mod = f"l{i}", mods[i]
        if kind == "conv":
            out[mod + ".weight"], out[mod + ".bias"] = params[n + ".kernel"], params[n + ".bias"]
        elif kind == "gn":
            out[mod + ".weight"], out[mod + ".bias"] = params[n + ".weight"], params[n + ".bias"]
        elif kind == "res":
            for ours, theirs in _VRES:
                out[f"{mod}.{theirs}"] = params[f"{n}.{ours}"]
            w = params.get(n + ".res_conv_layer.kernel")
            if w is not None and w.shape[0] != w.shape[1]:
                for ours, theirs in _VRES_SKIP:
                    out[f"{mod}.{theirs}"] = params[f"{n}.{ours}"]
        else:
            q, k, v = np.split(np.asarray(params[n + ".attention.in_proj.weight"]), 3)
            bq, bk, bv = np.split(np.asarray(params[n + ".attention.in_proj.bias"]), 3)
            for x, w, b in (("to_q", q, bq), ("to_k", k, bk), ("to_v", v, bv)):
                out[f"{mod}.{x}.weight"], out[f"{mod}.{x}.bias"] = w, b
            out[mod + ".to_out.0.weight"], out[mod + ".to_out.0.bias"] = params[n + ".attention.out_proj.weight"], params[n + ".attention.out_proj.bias"]
            out[mod + ".group_norm.weight"], out[mod + ".group_norm.bias"] = params[n + ".group_norm.weight"], params[n + ".group_norm.bias"]
    return out


def load_vae(path_or_state, which="decoder", ctx=None):
    """tsd.Decoder / tsd.Encoder (variant "*_torch") from a diffusers AutoencoderKL safetensors file
    (`vae/diffusion_pytorch_model.safetensors`) or an in-memory state dict."""
    from .model import param_specs
    from .vae import Decoder, Encoder
    state = read_safetensors(path_or_state) if isinstance(path_or_state, str) else path_or_state
    params = diffusers_vae_to_params(state, which)
    for name, shape, used, _ in param_specs(which + "_torch"):
        if name not in params:
            if used:
                raise KeyError(f"checkpoint has no tensor for {name}")
            params[name] = np.zeros(shape, np.float32)
    return (Decoder if which == "decoder" else Encoder)(ctx=ctx, params=params, variant=which + "_torch")


# ---- scheduler_config.json (diffusers) -> the keywords of `generate` / `generate_stream` ---------------------------------------------
def read_scheduler_config(path):
    """A diffusers scheduler_config.json -> {"prediction", "zero_terminal_snr", "spacing", "num_training_steps"}, the keywords `generate`
    and `generate_stream` take (the sampler itself is the caller's choice).  Reads prediction_type ("epsilon" | "v_prediction"),
    rescale_betas_zero_snr, timestep_spacing ("leading" | "trailing") and num_train_timesteps; a missing key has diffusers' default.
    ValueError for what the engine does not have: another beta schedule than "scaled_linear", other beta_start / beta_end than 0.00085 /
    0.012 (the one table, `tsd.alphas_cumprod`), trained_betas, "sample" prediction, "linspace" spacing."""
    with open(path, "r", encoding="utf-8") as f:
        cfg = json.load(f)
    if not isinstance(cfg, dict):
        raise ValueError(f"{path}: a scheduler config is a JSON object")
    sched = cfg.get("beta_schedule", "scaled_linear")
    if sched != "scaled_linear":
        raise ValueError(f"{path}: beta_schedule {sched!r} is not supported (the engine's table is 'scaled_linear')")
    if cfg.get("trained_betas") is not None:
        raise ValueError(f"{path}: trained_betas is not supported (the engine's table is scaled_linear 0.00085 .. 0.012)")
    b0, b1 = cfg.get("beta_start", 0.00085), cfg.get("beta_end", 0.012)
    if abs(float(b0) - 0.00085) > 1e-12 or abs(float(b1) - 0.012) > 1e-12:
        raise ValueError(f"{path}: beta_start / beta_end {b0} / {b1} are not supported (the engine's table is 0.00085 .. 0.012)")
    pred = {"epsilon": "epsilon", "v_prediction": "v"}.get(cfg.get("prediction_type", "epsilon"))
    if pred is None:
        raise ValueError(f"{path}: prediction_type {cfg.get('prediction_type')!r} is not supported ('epsilon' or 'v_prediction')")
    spacing = cfg.get("timestep_spacing", "leading")
    if spacing not in ("leading", "trailing"):
        raise ValueError(f"{path}: timestep_spacing {spacing!r} is not supported ('leading' or 'trailing')")
    n_train = cfg.get("num_train_timesteps", 1000)
    if not isinstance(n_train, int) or isinstance(n_train, bool) or n_train <= 0:
        raise ValueError(f"{path}: num_train_timesteps {n_train!r} is not a positive integer")
    return {"prediction": pred, "zero_terminal_snr": bool(cfg.get("rescale_betas_zero_snr", False)), "spacing": spacing,
            "num_training_steps": n_train}
