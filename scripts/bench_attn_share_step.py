"""What shared self attention (tsd_model_set_attn_share) does to a denoise step, and that a step without a table costs what it did:
interleaved same-box rounds, a fresh process per measurement, median and range.

  python scripts/bench_attn_share_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Two configurations: the headline (Tiny-SD, B = 8, L = 64, CFG on) and
kind 6 at B = 4, L = 64, CFG on; 50 seeded DDPM steps each.  Every round runs, per configuration and in an order that rotates from round
to round, the parent tree's step() twice, this tree's step() with no table and with share = (-1, 0, ..., 0) over the session's batch on
all levels (both CFG halves share, each inside its own half).  Each process times P passes of the enqueued steps with hipEvents (after a warm-up pass) and reports their median.  Every process has its own time limit and the first failure ends the run.  Recorded per configuration:
  (a) the parent against the parent: the A/A spread of this box;
  (b) this tree with no table against the parent's median - ACCEPTANCE: the median ratio lies inside (a)'s spread;
  (c) reported, not gated: the sharing arm against no table; and `calls`, the shared attention call (d = 40, B = 8, H = 8, S = 4096 and
      1024: seven of eight samples walk 2 S keys) beside the plain S x S and S x 2 S calls; the expectation is 7 / 8 of the S x 2 S call
      plus 1 / 8 of the S x S call.  These come from one process (the median of three timings of 20 launches), not interleaved.
Writes FILE (default profiles/attn_share_step_pairs.json); exits 1 when (b) is outside the floor at either configuration.

  python scripts/bench_attn_share_step.py --worker --root DIR --variant V --B B --L L [--share] | --worker --calls"""
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
ap.add_argument("--calls", action="store_true")
ap.add_argument("--root", default=ROOT)
ap.add_argument("--variant", default="diffusion")
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--L", type=int, default=64)
ap.add_argument("--share", action="store_true", help="worker: share = (-1, 0, ..., 0) over B samples (absent: no table is set - the parent's library is never asked for it)")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_share_step_pairs.json"))
a = ap.parse_args()
SEED, T = 1234, 77
CONFIGS = {"headline_tiny_B8_L64": ("diffusion", 8, 64), "kind6_B4_L64": ("diffusion_sd15_torch", 4, 64)}


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    dctx = tsd.default_context()
    if a.calls:  # us per call, median of three timings of 20 launches each
        lib, ms, out = tsd._lib.lib(), C.c_float(0), {}
        for name, (S, Sk, share) in {"plain_4096x4096": (4096, 4096, 0), "plain_4096x8192": (4096, 8192, 0), "shared_4096_7of8": (4096, 4096, 1),
                                     "plain_1024x1024": (1024, 1024, 0), "plain_1024x2048": (1024, 2048, 0), "shared_1024_7of8": (1024, 1024, 1)}.items():
            v = []
            for _ in range(3):
                if S == Sk:
                    tsd._lib.check(lib.tsd_debug_attn_bench_share(dctx.h, 8, 8, 40, S, share, 20, C.byref(ms)))
                else:
                    tsd._lib.check(lib.tsd_debug_attn_bench(dctx.h, 8, 8, 40, S, Sk, 20, C.byref(ms)))
                v.append(1e3 * ms.value)
            out[name] = round(float(np.median(v)), 2)
        print(json.dumps({"lib": tsd._lib.LIB_PATH, "us_per_call": out}))
        return
    B, L = a.B, a.L
    unet = tsd.Diffusion(seed=SEED, variant=a.variant)
    if a.share:
        unet.set_attn_share((-1,) + (0,) * (B - 1))
    W = 1024 if a.variant == "diffusion_sd2" else 768
    lat = rng.normal(SEED, 4, B * 4 * L * L).reshape(B, 4, L, L).astype(np.float32)
    ctx, uctx = (rng.normal(SEED, s, B * T * W).reshape(B, T, W) for s in (5, 6))
    sess = tsd.Session(unet.model, None, B, L, T, cfg=True)
    sess.set_schedule(1000, a.steps, 0)
    n, ms = sess.num_steps, []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        sess.upload(lat, ctx, uctx, None, 7.5)
        sess.set_seeds([100 + b for b in range(B)])
        sess.add_noise_seeded(0)
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    assert np.isfinite(sess.latents()).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "share": a.share, "ms_per_step": [round(v, 4) for v in ms], "median": round(float(np.median(ms)), 4)}))


def measure(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)] + args
    env = {k: val for k, val in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {root} {args} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} {args} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def pair(on, off):
    r = [x / y for x, y in zip(on, off)]
    d = [1e3 * (x - y) for x, y in zip(on, off)]
    return {"ratio_per_round": [round(v, 5) for v in r], "ratio_median": round(float(np.median(r)), 5), "ratio_range": spread(r),
            "us_per_step_per_round": [round(v, 1) for v in d], "us_per_step_median": round(float(np.median(d)), 1)}


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = []
    for cfg, (variant, B, L) in CONFIGS.items():
        base = ["--variant", variant, "--B", str(B), "--L", str(L)]
        arms += [(f"{cfg}/parent_1", a.parent_root, base), (f"{cfg}/parent_2", a.parent_root, base), (f"{cfg}/none", ROOT, base),
                 (f"{cfg}/share", ROOT, base + ["--share"])]
    t0, rounds = time.time(), []
    calls = measure(ROOT, ["--calls"])["us_per_call"]
    for r in range(a.rounds):
        k = r % len(arms)
        rec = {name: measure(root, args) for name, root, args in arms[k:] + arms[:k]}
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    out = {"what": "ms per step(), CFG on, 50 seeded DDPM steps; interleaved same-box rounds, one fresh process per measurement",
           "rounds": len(rounds), "passes": a.passes, "configurations": {}, "attention_call_us": calls}
    ok = True
    for cfg in CONFIGS:
        p1, p2 = med[f"{cfg}/parent_1"], med[f"{cfg}/parent_2"]
        aa = [y / x for x, y in zip(p1, p2)]
        lo, hi = min(aa + [1.0 / v for v in aa]), max(aa + [1.0 / v for v in aa])
        pm = float(np.median(p1 + p2))
        rb = [v / pm for v in med[f"{cfg}/none"]]
        inside = bool(lo <= float(np.median(rb)) <= hi)
        ok = ok and inside
        out["configurations"][cfg] = {"a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
                                      "b_no_table_over_parent_median": {"parent_median_ms": round(pm, 4), "per_round": [round(v, 5) for v in rb],
                                                                        "median": round(float(np.median(rb)), 5), "inside_floor": inside},
                                      "c_share_over_none": pair(med[f"{cfg}/share"], med[f"{cfg}/none"])}
    out.update({"ms_per_step": med, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S")})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"configurations": out["configurations"], "attention_call_us": calls}))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
