"""What swapping a LoRA adapter costs on the SD-1.x UNet (kind diffusion_sd15_torch, random init): the device merge against the only
route the library offered before it - merging on the host from fp32 copies of the weights and pushing every touched tensor through
`tsd_model_set_param` again.

  python scripts/bench_lora_swap.py [--rank 16] [--rounds 5] [--out FILE]

The adapter is the one tests/test_gpu_lora.py loads: for all 16 attention blocks attn1 / attn2 to_q, to_k, to_v, to_out.0,
ff.net.0.proj, ff.net.2, proj_in, proj_out, and one resnet conv1 (193 pairs, 161 parameters), alpha = 2.  One process, one model;
every round measures the three arms one after the other, in an order that rotates from round to round, wall time around the calls
including `tsd_model_prepare` (the derived buffers a forward needs):
  device_add    load_lora(state, unet) + prepare
  device_clear  lora_clear() + prepare
  host_add      numpy fp32  W + s * up @ down  per row block from host copies of the base, set_param of each touched parameter, prepare
                (the host copies are read back before the timing starts: a user of that route has to keep them, 4 bytes per weight)
After host_add the base is restored with set_param outside the timing.  Writes FILE (default profiles/lora_swap_pairs.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "stable-diffusion.mojo_amd"))
ap = argparse.ArgumentParser()
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_swap_pairs.json"))
a = ap.parse_args()
ALPHA = 2.0


def main():
    import tsd
    from tsd.checkpoint import SD15_MODULES
    tsd.set_strict(True)
    unet = tsd.Diffusion(seed=5, variant="diffusion_sd15_torch")
    m = unet.model
    targets = tsd.lora_targets("diffusion_sd15_torch")
    shapes = {n: s for n, s, _, _ in m.specs}
    suffixes = ["proj_in", "proj_out"] + ["transformer_blocks.0." + s for s in (
        "attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
        "ff.net.0.proj", "ff.net.2")]
    mods = [f"{b}.{s}" for b in SD15_MODULES if ".attentions." in b for s in suffixes] + ["down_blocks.2.resnets.0.conv1"]
    g = np.random.default_rng(21)
    state, pairs = {}, {}
    for mod in mods:
        pname, _, rows = targets[mod]
        shape = shapes[pname]
        down = (0.05 * g.standard_normal((a.rank,) + tuple(shape[1:]))).astype(np.float32)
        up = (0.05 * g.standard_normal((rows, a.rank) + ((1, 1) if len(shape) == 4 else ()))).astype(np.float32)
        stem = "lora_unet_" + mod.replace(".", "_")
        state[stem + ".lora_down.weight"], state[stem + ".lora_up.weight"], state[stem + ".alpha"] = down, up, np.float32(ALPHA)
        pairs[mod] = (down.reshape(a.rank, -1), up.reshape(rows, a.rank))
    touched = sorted({targets[mod][0] for mod in mods})
    base = {p: m.get_param(p) for p in touched}   # the fp32 copies the host route needs
    m.prepare()
    s = ALPHA / a.rank

    def device_add():
        res = tsd.load_lora(state, unet=unet)
        m.prepare()
        assert res["applied"] == len(mods) and m.lora_count == len(touched)

    def device_clear():
        m.lora_clear()
        m.prepare()
        assert m.lora_count == 0

    def host_add():
        for p in touched:
            W = base[p].reshape(base[p].shape[0], -1).copy()
            for mod in mods:
                if targets[mod][0] == p:
                    _, row0, rows = targets[mod]
                    down, up = pairs[mod]
                    W[row0:row0 + rows] += np.float32(s) * (up @ down)
            m.set_param(m.param_index(p), W.reshape(base[p].shape))
        m.prepare()

    def host_restore():
        for p in touched:
            m.set_param(m.param_index(p), base[p])
        m.prepare()

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    device_add(); device_clear(); host_add(); host_restore()   # warm-up: staging buffers, derived allocations, numpy's threads
    t = {"device_add": [], "device_clear": [], "host_add": []}
    for r in range(a.rounds):
        if r % 2 == 0:
            t["device_add"].append(timed(device_add)); t["device_clear"].append(timed(device_clear))
            t["host_add"].append(timed(host_add)); host_restore()
        else:
            t["host_add"].append(timed(host_add)); host_restore()
            t["device_add"].append(timed(device_add)); t["device_clear"].append(timed(device_clear))
        print(f"round {r}: " + "  ".join(f"{k} {v[-1]:.3f} s" for k, v in t.items()), flush=True)
    out = {"what": "wall seconds to swap a rank-%d adapter (%d pairs, %d parameters, %.1f M weights) on the SD-1.x UNet, tsd_model_prepare included; "
                   "one process, arms alternate order from round to round" % (a.rank, len(mods), len(touched), sum(base[p].size for p in touched) / 1e6),
           "rounds": a.rounds,
           "seconds": {k: {"per_round": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "min": round(min(v), 4),
                           "max": round(max(v), 4)} for k, v in t.items()},
           "host_over_device_per_round": [round(h / d, 3) for h, d in zip(t["host_add"], t["device_add"])],
           "date": time.strftime("%Y-%m-%d %H:%M:%S")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("seconds", "host_over_device_per_round")}))
    m.close()


if __name__ == "__main__":
    main()
