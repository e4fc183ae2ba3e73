"""fp64 restatement of the IP-Adapter Plus image projection (model kind "ip_adapter_plus_sd15"): the Perceiver resampler
`Resampler(dim=768, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=768, ff_mult=4)` of the published
IP-Adapter code, written from memory of that module (no file and no network here to check it against), on the parameter names the model
keeps.  It takes the parameters as the engine holds them (`Model.get_param`: every weight an fp16 value), so what a test measures is the
device's arithmetic, not the rounding of the weights.

    x   = hidden . proj_in^T + b_in                              [S][768]
    lat = latents                                                [16][768]
    4 x:  xn = LN(x; norm1)   ln = LN(lat; norm2)
          q = ln . Wq^T       kv = concat(xn, ln) . Wkv^T        k = kv[:, :768], v = kv[:, 768:]
          per head of 64 columns  P = softmax(q k^T / 8) over all S + 16 keys,  a = P v
          lat = a . Wo^T + lat
          lat = gelu_erf(LN(lat; ff_norm) . W1^T) . W2^T + lat
    tokens = LN(lat . proj_out^T + b_out; norm_out)              [16][768]

NEAR_MISSES are the restatements one slip away, kept so that tests can show the tolerance separates them from the module: they move the
result by far more than the whole-model tolerance on the test draw (tests/test_ipplus_cpu.py asserts more than 10 TOL_MODEL at S = 5 and
49).  A tanh-GELU in place of the erf-GELU does NOT belong to that list: it moves the result by a few 1e-4, which no model-level test can
see; the GELU kernel has its own element-wise test."""
import numpy as np

from oracle import rng

DIM, DEPTH, HEADS, DHEAD, QUERIES, EMBED, FF = 768, 4, 12, 64, 16, 1280, 3072
N_PARAMS, N_ELEMENTS, N_ELEMENTS_IMAGE_PROJ = 83, 49087488, 29918208
NEAR_MISSES = ("no_latent_keys", "scale_once", "kv_swapped", "norms_swapped", "no_norm_out")
TABLE_WIDTHS = (320, 320, 640, 640, 1280, 1280, 1280) + (1280,) * 3 + (640,) * 3 + (320,) * 3   # 6 down, mid, 9 up: the step table's order


def published_index(t):
    """`ip_adapter.<i>` of the t-th cross-attention block of the step table (6 down, 1 mid, 9 up)."""
    return 2 * t + 1 if t < 6 else (31 if t == 6 else 2 * t - 1)


def inventory():
    """[(name, shape)] of the 83 parameters in the model's order: the resampler's state-dict order, then the 16 pairs in the step table's."""
    out = [("image_proj.latents", (1, QUERIES, DIM)), ("image_proj.proj_in.weight", (DIM, EMBED)), ("image_proj.proj_in.bias", (DIM,)),
           ("image_proj.proj_out.weight", (DIM, DIM)), ("image_proj.proj_out.bias", (DIM,)),
           ("image_proj.norm_out.weight", (DIM,)), ("image_proj.norm_out.bias", (DIM,))]
    for l in range(DEPTH):
        n = f"image_proj.layers.{l}."
        out += [(n + "0.norm1.weight", (DIM,)), (n + "0.norm1.bias", (DIM,)), (n + "0.norm2.weight", (DIM,)), (n + "0.norm2.bias", (DIM,)),
                (n + "0.to_q.weight", (HEADS * DHEAD, DIM)), (n + "0.to_kv.weight", (2 * HEADS * DHEAD, DIM)), (n + "0.to_out.weight", (DIM, HEADS * DHEAD)),
                (n + "1.0.weight", (DIM,)), (n + "1.0.bias", (DIM,)), (n + "1.1.weight", (FF, DIM)), (n + "1.3.weight", (DIM, FF))]
    for t, C in enumerate(TABLE_WIDTHS):
        out += [(f"ip_adapter.{published_index(t)}.to_k_ip.weight", (C, DIM)), (f"ip_adapter.{published_index(t)}.to_v_ip.weight", (C, DIM))]
    return out


def _is_norm(name):
    import re
    return ".norm" in name or re.search(r"layers\.\d+\.1\.0\.(weight|bias)$", name) is not None   # layers.L.1.0 is the feed-forward LayerNorm


def draw_params(seed=0, specs=None):
    """The test draw: linear weights N(0, 1 / fan_in), latents N(0, 1 / 768), norm weights 1 + 0.1 n, norm biases 0.1 n, linear biases
    0.02 n, n standard normal from the oracle's counter RNG (one stream per parameter)."""
    out = {}
    for i, (name, shape) in enumerate(specs or inventory()):
        n = rng.normal(seed, 4000 + i, int(np.prod(shape))).reshape(shape).astype(np.float64)
        if _is_norm(name):
            v = 1.0 + 0.1 * n if name.endswith(".weight") else 0.1 * n
        elif name.endswith(".bias"):
            v = 0.02 * n
        else:
            v = n / np.sqrt(shape[-1])
        out[name] = v.astype(np.float32)
    return out


def _ln(x, w, b, eps=1e-5):
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def _gelu_erf(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def resample(P, hidden, miss=None, spreads=None):
    """One sample: hidden [S][1280] -> tokens fp64 [16][768].  miss: None, or one of NEAR_MISSES.  spreads: a list that receives the
    smallest per-row score spread (max - min over the keys) of every layer."""
    assert miss is None or miss in NEAR_MISSES
    p = lambda k: np.asarray(P["image_proj." + k], np.float64)  # noqa: E731
    x = np.asarray(hidden, np.float64) @ p("proj_in.weight").T + p("proj_in.bias")
    lat = p("latents").reshape(QUERIES, DIM)
    for l in range(DEPTH):
        n = f"layers.{l}."
        n1, n2 = ("0.norm2", "0.norm1") if miss == "norms_swapped" else ("0.norm1", "0.norm2")
        xn = _ln(x, p(n + n1 + ".weight"), p(n + n1 + ".bias"))
        ln = _ln(lat, p(n + n2 + ".weight"), p(n + n2 + ".bias"))
        q = ln @ p(n + "0.to_q.weight").T
        kv = (xn if miss == "no_latent_keys" else np.concatenate([xn, ln])) @ p(n + "0.to_kv.weight").T
        k, v = (kv[:, DIM:], kv[:, :DIM]) if miss == "kv_swapped" else (kv[:, :DIM], kv[:, DIM:])
        a = np.empty_like(q)
        for h in range(HEADS):
            c = slice(h * DHEAD, (h + 1) * DHEAD)
            s = q[:, c] @ k[:, c].T * (DHEAD ** -0.25 if miss == "scale_once" else 1.0 / 8.0)
            if spreads is not None:
                spreads.append(float((s.max(-1) - s.min(-1)).min()))
            e = np.exp(s - s.max(-1, keepdims=True))
            a[:, c] = (e / e.sum(-1, keepdims=True)) @ v[:, c]
        lat = a @ p(n + "0.to_out.weight").T + lat
        f = _ln(lat, p(n + "1.0.weight"), p(n + "1.0.bias"))
        lat = _gelu_erf(f @ p(n + "1.1.weight").T) @ p(n + "1.3.weight").T + lat
    y = lat @ p("proj_out.weight").T + p("proj_out.bias")
    return y if miss == "no_norm_out" else _ln(y, p("norm_out.weight"), p("norm_out.bias"))


def resample_batch(P, hidden, miss=None):
    """hidden [B][S][1280] -> fp64 [B][16][768]."""
    return np.stack([resample(P, h, miss) for h in np.asarray(hidden)])


def hidden_states(B, S, tag, seed=7):
    """Test input: N(0, 1) rows, fp32 [B][S][1280]."""
    return rng.normal(seed, tag, B * S * EMBED).reshape(B, S, EMBED).astype(np.float32)


def f16_weights(P):
    """The draw as a model holds it: matrices (and the latents) rounded to fp16, vectors (biases, norm parameters) kept in fp32."""
    return {k: (v.astype(np.float16).astype(np.float32) if v.ndim >= 2 else v) for k, v in P.items()}
