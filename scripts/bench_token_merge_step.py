"""What token merging (tsd_model_set_token_merge) does to a denoise step beside windowing, and that a step without a table costs what it
did: interleaved same-box rounds, a fresh process per measurement, median and range (the discipline of bench_attn_window_step.py).

  python scripts/bench_token_merge_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Configurations, CFG on, 50 seeded DDPM steps: the headline (Tiny-SD, B = 8,
L = 64 - a merged block loses its fused head kernel there) and kind 6 at B = 4, L = 64, each with the parent twice, this tree with no table,
with ratio = (0.5, 0, 0, 0) and with win = (32, 0, 0, 0); kind 6 at B = 1, L = 96 (level 1 is 48 x 48: 32 does not divide it, merging needs
no divisor) with no table, ratio = (0.5, 0.5, 0, 0) and win = (32, 16, 0, 0).  The order rotates from round to round.  Recorded:
  (a) the parent against the parent: the A/A spread of this box;
  (b) this tree with no table against the parent's median - ACCEPTANCE: the median ratio lies inside (a)'s spread;
  (c) reported, not gated: merge and window against none, and `classes`: per kernel class the milliseconds and launches of ONE profiled
      kind-6 forward (B = 8, L = 64) with no table and with ratio 0.5 - the elementwise difference is the plan, merge and unmerge launches.
Writes FILE (default profiles/token_merge_step_pairs.json); exits 1 when (b) is outside the floor.

  python scripts/bench_token_merge_step.py --worker --root DIR --variant V --B B --L L [--tome a,b,c,d | --win a,b,c,d] [--classes]"""
import argparse
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
ap.add_argument("--classes", action="store_true")
ap.add_argument("--root", default=ROOT)
ap.add_argument("--variant", default="diffusion")
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--L", type=int, default=64)
ap.add_argument("--tome", default=None, help="worker: the ratio table (absent: none is set - the parent's library is never asked for it)")
ap.add_argument("--win", default=None)
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_merge_step_pairs.json"))
a = ap.parse_args()
SEED, T = 1234, 77
CONFIGS = {"headline_tiny_B8_L64": ("diffusion", 8, 64), "kind6_B4_L64": ("diffusion_sd15_torch", 4, 64)}


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    dctx, B, L = tsd.default_context(), a.B, a.L
    unet = tsd.Diffusion(seed=SEED, variant=a.variant)
    if a.tome is not None:
        unet.set_token_merge(tuple(float(v) for v in a.tome.split(",")))
    if a.win is not None:
        unet.set_attn_window(tuple(int(v) for v in a.win.split(",")))
    lat = rng.normal(SEED, 4, B * 4 * L * L).reshape(B, 4, L, L).astype(np.float32)
    ctx, uctx = (rng.normal(SEED, s, B * T * 768).reshape(B, T, 768) for s in (5, 6))
    if a.classes:  # one profiled forward at the UNet's batch, after a warm-up forward
        temb = np.repeat(tsd.get_time_embedding(500.0).reshape(1, 320), B, axis=0)
        unet.forward(lat, ctx, temb)
        dctx.profile_begin()
        unet.forward(lat, ctx, temb)
        print(json.dumps({"lib": tsd._lib.LIB_PATH, "classes": {k: [round(v[0], 4), v[1]] for k, v in dctx.profile_end().items() if v[1]}}))
        return
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
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "ms_per_step": [round(v, 4) for v in ms], "median": round(float(np.median(ms)), 4)}))


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


def pair(on, off):
    r = [x / y for x, y in zip(on, off)]
    d = [1e3 * (x - y) for x, y in zip(on, off)]
    return {"ratio_per_round": [round(v, 5) for v in r], "ratio_median": round(float(np.median(r)), 5),
            "ratio_range": [round(min(r), 5), round(max(r), 5)], "us_per_step_median": round(float(np.median(d)), 1)}


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = []
    for cfg, (variant, B, L) in CONFIGS.items():
        base = ["--variant", variant, "--B", str(B), "--L", str(L)]
        arms += [(f"{cfg}/parent_1", a.parent_root, base), (f"{cfg}/parent_2", a.parent_root, base), (f"{cfg}/none", ROOT, base),
                 (f"{cfg}/tome", ROOT, base + ["--tome", "0.5,0,0,0"]), (f"{cfg}/win32", ROOT, base + ["--win", "32,0,0,0"])]
    base = ["--variant", "diffusion_sd15_torch", "--B", "1", "--L", "96"]
    arms += [("kind6_B1_L96/none", ROOT, base), ("kind6_B1_L96/tome", ROOT, base + ["--tome", "0.5,0.5,0,0"]),
             ("kind6_B1_L96/win32", ROOT, base + ["--win", "32,16,0,0"])]
    t0, rounds = time.time(), []
    prof = ["--variant", "diffusion_sd15_torch", "--B", "8", "--L", "64", "--classes"]
    classes = {"none": measure(ROOT, prof)["classes"], "tome_0.5": measure(ROOT, prof + ["--tome", "0.5,0,0,0"])["classes"]}
    for r in range(a.rounds):
        k = r % len(arms)
        rec = {name: measure(root, args) for name, root, args in arms[k:] + arms[:k]}
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    out = {"what": "ms per step(), CFG on, 50 seeded DDPM steps; interleaved same-box rounds, one fresh process per measurement",
           "rounds": len(rounds), "passes": a.passes, "configurations": {}, "classes_ms_launches_one_forward_kind6_B8_L64": classes}
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
                                      "c_tome_over_none": pair(med[f"{cfg}/tome"], med[f"{cfg}/none"]),
                                      "c_win32_over_none": pair(med[f"{cfg}/win32"], med[f"{cfg}/none"])}
    L96 = "kind6_B1_L96"
    out["configurations"][L96] = {"none_ms": round(float(np.median(med[f"{L96}/none"])), 4), "tome_table": "0.5,0.5,0,0", "win_table": "32,16,0,0",
                                  "c_tome_over_none": pair(med[f"{L96}/tome"], med[f"{L96}/none"]),
                                  "c_win_over_none": pair(med[f"{L96}/win32"], med[f"{L96}/none"])}
    out.update({"ms_per_step": med, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S")})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"configurations": out["configurations"], "classes": classes}))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
