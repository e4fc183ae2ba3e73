"""That a square denoise step costs what it did before sessions could be rectangular, and what a rectangular step costs: interleaved
same-box rounds at B = 8, CFG on, 50 seeded DDPM steps.

  python scripts/bench_rect_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs five fresh processes one after the other, in an order
that rotates from round to round: the parent tree's step() at 64x64 twice, this tree's step() at 64x64, at 64x96 and at 96x64 (latent
rows x columns: 512x768 and 768x512 pixels).  Each process times P passes of the 50 enqueued steps with hipEvents on the library's stream
(after one warm-up pass) and reports their median.  Recorded:
  floor the parent against the parent, the A/A spread of this box (the pair noise floor);
  (a) this tree's square step() against the parent's - the same launches through the LH == LW case of the rectangular code;
  (b) 64x96 and 96x64: ms per step, and per token relative to this tree's 64x64 (6144 tokens against 4096).  Informational.
Writes FILE (default profiles/rect_step_pairs.json).  No threshold: the ratios and their ranges are the result.

  python scripts/bench_rect_step.py --worker --root DIR --shape 64x96     one measurement, one JSON line (what the driver starts)"""
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
ap.add_argument("--root", default=ROOT)
ap.add_argument("--shape", default="64x64")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=4)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_step_pairs.json"))
a = ap.parse_args()
SEED, B, T = 1234, 8, 77


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    LH, LW = (int(v) for v in a.shape.split("x"))
    unet = tsd.Diffusion(seed=SEED)
    dctx = tsd.default_context()
    lat = np.zeros((B, 4, LH, LW), dtype=np.float32)
    ctx = rng.normal(SEED, 5, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(SEED, 6, B * T * 768).reshape(B, T, 768)
    seeds = list(range(100, 100 + B))
    sess = tsd.Session(unet.model, None, B, LH if LH == LW else (LH, LW), T, cfg=True)   # the parent tree takes a side only
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    ms = []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        sess.upload(lat, ctx, uctx, None, 7.5)
        sess.set_seeds(seeds)
        sess.seed_latents()
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    out = sess.latents()
    assert out.shape == (B, 4, LH, LW) and np.isfinite(out).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "shape": [LH, LW], "ms_per_step": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4)}))


def measure(root, shape):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--shape", shape, "--passes", str(a.passes),
           "--steps", str(a.steps)]
    env = {k: v for k, v in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} {shape} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, "64x64"), ("parent_2", a.parent_root, "64x64"), ("new_64x64", ROOT, "64x64"),
            ("new_64x96", ROOT, "64x96"), ("new_96x64", ROOT, "96x64")]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, root, shape in arms[k:] + arms[:k]:
            rec[name] = measure(root, shape)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {k: [rd[k]["median"] for rd in rounds] for k, _, _ in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    ra = [s / p for s, p in zip(med["new_64x64"], med["parent_1"])]
    rect = {}
    for name, tokens in (("new_64x96", 64 * 96), ("new_96x64", 96 * 64)):
        per_tok = [(m / tokens) / (s / 4096.0) for m, s in zip(med[name], med["new_64x64"])]
        rect[name[4:]] = {"ms_per_step_median": round(float(np.median(med[name])), 4), "ms_per_step_range": spread(med[name]),
                          "per_token_over_64x64": {"per_round": [round(v, 5) for v in per_tok], "median": round(float(np.median(per_tok)), 5),
                                                   "range": spread(per_tok)}}
    out = {
        "what": "ms per denoise step, B=8 CFG on, 50 seeded DDPM steps; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "floor_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "a_new_square_step_over_parent_step": {"per_round": [round(v, 5) for v in ra], "median": round(float(np.median(ra)), 5),
                                               "range": spread(ra), "inside_floor": bool(lo <= float(np.median(ra)) <= hi)},
        "b_rectangular": rect,
        "c_ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("floor_parent_over_parent", "a_new_square_step_over_parent_step", "b_rectangular")}))


if __name__ == "__main__":
    worker() if a.worker else driver()
