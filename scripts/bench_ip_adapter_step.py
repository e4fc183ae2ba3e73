"""What an IP-Adapter costs a denoise step of the full-size UNet, and that a plain step costs what it did: interleaved same-box rounds at
B = 4, L = 64, CFG on, 50 seeded DDPM steps (the pattern of scripts/bench_control_step.py).

  python scripts/bench_ip_adapter_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs four fresh processes one after the other, in an order
that rotates from round to round: the parent tree's step() twice, then this tree's step() without an adapter and with one (scale 1 on both
CFG halves, N = 4 tokens).  Each process times P passes of the 50 enqueued steps with hipEvents on the library's stream (after one warm-up
pass) and reports their median.  Every process has its own time limit and the first failure ends the run.  Recorded:
  (a) the parent against the parent, the A/A spread of this box (the pair noise floor);
  (b) this tree's plain step() against the parent's median - ACCEPTANCE: the median ratio lies inside (a)'s spread (nothing existing
      got slower);
  (c) the adapted step() at scale 1 against the plain one, as a ratio and in us per step - reported, not gated (16 launches of
      k_ip_attn_add, and the six C = 320 blocks leave their fused head / tail kernels for the op-by-op path);
  (d) k_ip_attn_add alone (tsd_debug_ip_attn_bench, this tree) at the three level shapes S = 4096 / 1024 / 256 with 8 samples, 8 heads of
      40 / 80 / 160 and N = 4, in us and as a fraction of the 3 M C 2-byte floor at the 8 TB/s HBM peak; and beside it, on the PARENT's
      library, tsd_debug_attn_bench at the same (B, H, d, Sq) with Sk = 16 - the flash call the composed alternative would make, before
      its axpy.  Reported, not gated: where the new launch is not faster, both numbers stand.
Writes FILE (default profiles/ip_adapter_step_pairs.json); exits 1 when (b) is outside the floor.

  python scripts/bench_ip_adapter_step.py --worker --root DIR [--adapter SCALE]     one step measurement, one JSON line
  python scripts/bench_ip_adapter_step.py --kernel-worker --root DIR --which ip|flash   the (d) launches of one library, one JSON line"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--worker", action="store_true")
ap.add_argument("--kernel-worker", action="store_true")
ap.add_argument("--which", default="ip")
ap.add_argument("--root", default=ROOT)
ap.add_argument("--adapter", type=float, default=None, help="worker: set_ip_adapter with this scale (absent: no adapter)")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_adapter_step_pairs.json"))
a = ap.parse_args()
SEED, B, L, T, N_TOK = 1234, 4, 64, 77, 4
HBM_PEAK_GBS = 8000.0
LEVELS = ((4096, 40), (1024, 80), (256, 160))   # (S, head dim) of the three attention levels at L = 64; 8 heads, 2B = 8 samples


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    unet = tsd.Diffusion(seed=SEED, variant="diffusion_sd15")
    dctx = tsd.default_context()
    lat = rng.normal(SEED, 4, B * 4 * L * L).reshape(B, 4, L, L).astype(np.float32)
    ctx = rng.normal(SEED, 5, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(SEED, 6, B * T * 768).reshape(B, T, 768)
    sess = tsd.Session(unet.model, None, B, L, T, cfg=True)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    ip = tok = utok = None
    if a.adapter is not None:  # the parent's library is never asked for what it does not have
        ip = tsd.IPAdapter(seed=SEED)
        emb = rng.normal(SEED, 7, B * 1024).reshape(B, 1024)
        tok, utok = ip.project(emb), ip.project(np.zeros_like(emb))
    ms = []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        sess.upload(lat, ctx, uctx, None, 7.5)
        sess.set_seeds([100 + b for b in range(B)])
        sess.add_noise_seeded(0)
        if ip is not None and p == 0:
            sess.set_ip_adapter(ip, tok, utok, scale=a.adapter)   # it outlives the later uploads
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    assert np.isfinite(sess.latents()).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "adapter": a.adapter, "ms_per_step": [round(v, 4) for v in ms], "median": round(float(np.median(ms)), 4)}))


def kernel_worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    tsd.set_strict(True)
    dctx = tsd.default_context()
    lib = tsd._lib.lib()
    out = {}
    for S, hd in LEVELS:
        ms = C.c_float(0.0)
        if a.which == "ip":
            rc = lib.tsd_debug_ip_attn_bench(dctx.h, 2 * B, 8, hd, S, N_TOK, a.iters, C.byref(ms))
        else:
            rc = lib.tsd_debug_attn_bench(dctx.h, 2 * B, 8, hd, S, 16, a.iters, C.byref(ms))
        assert rc == 0, tsd._lib.last_error()
        out[f"S{S}_d{hd}"] = round(1e3 * ms.value, 3)
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "which": a.which, "us": out}))


def _run(cmd, root, what):
    env = {k: val for k, val in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {what} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {what} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def measure(root, adapter):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)] + \
        (["--adapter", repr(adapter)] if adapter is not None else [])
    return _run(cmd, root, f"{root} adapter={adapter}")


def measure_kernel(root, which):
    cmd = [sys.executable, os.path.abspath(__file__), "--kernel-worker", "--root", root, "--which", which, "--iters", str(a.iters)]
    return _run(cmd, root, f"{root} kernel {which}")["us"]


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, None), ("parent_2", a.parent_root, None), ("step_plain", ROOT, None), ("step_adapter", ROOT, 1.0)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, root, adapter in arms[k:] + arms[:k]:
            rec[name] = measure(root, adapter)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    rb = [v / parent_median for v in med["step_plain"]]
    inside = bool(lo <= float(np.median(rb)) <= hi)
    rc = [x / y for x, y in zip(med["step_adapter"], med["step_plain"])]
    dc = [1e3 * (x - y) for x, y in zip(med["step_adapter"], med["step_plain"])]
    ip_us = measure_kernel(ROOT, "ip")
    flash_us = measure_kernel(a.parent_root, "flash")
    kern = {}
    for S, hd in LEVELS:
        key = f"S{S}_d{hd}"
        floor_bytes = 3 * (2 * B * S) * (8 * hd) * 2
        floor_us = floor_bytes / (HBM_PEAK_GBS * 1e9) * 1e6
        kern[key] = {"k_ip_attn_add_us": ip_us[key], "floor_bytes": floor_bytes, "floor_us_at_hbm_peak": round(floor_us, 3),
                     "floor_over_measured": round(floor_us / ip_us[key], 4) if ip_us[key] > 0 else None,
                     "parent_flash_sk16_us": flash_us[key], "new_over_flash": round(ip_us[key] / flash_us[key], 4) if flash_us[key] > 0 else None}
    out = {
        "what": "ms per step(), full-size UNet, B=4 L=64 CFG on, 50 seeded DDPM steps; adapter arm: set_ip_adapter(scale 1, N = 4); interleaved "
                "same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "b_step_plain_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in rb],
                                            "median": round(float(np.median(rb)), 5), "range": spread(rb), "inside_floor": inside},
        "c_step_adapter_over_plain": {"per_round": [round(v, 5) for v in rc], "median": round(float(np.median(rc)), 5), "range": spread(rc),
                                      "us_per_step_added_median": round(float(np.median(dc)), 1), "us_per_step_added_range": spread(dc)},
        "d_kernel": kern,
        "ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_parent_over_parent", "b_step_plain_over_parent_median", "c_step_adapter_over_plain", "d_kernel")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    if a.worker:
        worker()
    elif a.kernel_worker:
        kernel_worker()
    else:
        driver()
