"""What FreeU costs a denoise step of the full-size UNet, and that a step with FreeU off costs what it did: interleaved same-box rounds
at B = 4, L = 64, CFG on, 50 seeded DDPM steps.

  python scripts/bench_freeu_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs seven fresh processes one after the other, in an order
that rotates from round to round: the parent tree's step() twice, then this tree's step() with FreeU off and with the paper's SD-1.x
values (b1 1.5, b2 1.6, s1 0.9, s2 0.2) under both conventions of tsd.freeu_table and both modes.  Each process times P passes of the 50
enqueued steps with hipEvents on the library's stream (after one warm-up pass) and reports their median.  Every process has its own time
limit and the first failure ends the run.  Recorded:
  (a) the parent against the parent: the A/A spread of this box (the pair noise floor);
  (b) this tree's step() with FreeU off against the parent's median - ACCEPTANCE: the median ratio lies inside (a)'s spread (an off model
      enqueues the launches it always did);
  (c) each FreeU arm against off, in us per step and as a ratio - reported, not gated: the launches themselves plus the statistics passes
      the rewritten tensors' GroupNorms now run on their own, since the producers' statistics are dropped.
Writes FILE (default profiles/freeu_step_pairs.json); exits 1 when (b) is outside the floor.

  python scripts/bench_freeu_step.py --worker --root DIR [--freeu CONVENTION --mode MODE]     one measurement, one JSON line"""
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
ap.add_argument("--freeu", default=None, help="worker: convention of tsd.freeu_table (absent: FreeU off)")
ap.add_argument("--mode", default="constant", choices=("constant", "modulated"))
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeu_step_pairs.json"))
a = ap.parse_args()
SEED, B, L, T = 1234, 4, 64, 77
VALUES = dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2)
# (Ch, Cr, divisor of the latent side) of the twelve decoder concats in pop order
CONCATS = ((1280, 1280, 8), (1280, 1280, 8), (1280, 1280, 8), (1280, 1280, 4), (1280, 1280, 4), (1280, 640, 4), (1280, 640, 2), (640, 640, 2),
           (640, 320, 2), (640, 320, 1), (320, 320, 1), (320, 320, 1))


def freeu_bytes(convention):
    """fp16 bytes the FreeU launches of one step read and write at the UNet's batch 2B: half of h read and written, r read twice and
    written once (the modulated mode reads all of h once more for the means)."""
    js = range(6) if convention == "diffusers" else range(10)
    return sum(2 * 2 * B * (L // d) * (L // d) * (ch + 3 * cr) for j, (ch, cr, d) in enumerate(CONCATS) if j in js)


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    unet = tsd.Diffusion(seed=SEED, variant="diffusion_sd15")
    if a.freeu is not None:  # the parent's library is never asked for what it does not have
        unet.set_freeu(convention=a.freeu, modulated=a.mode == "modulated", **VALUES)
    dctx = tsd.default_context()
    lat = rng.normal(SEED, 4, B * 4 * L * L).reshape(B, 4, L, L).astype(np.float32)
    ctx = rng.normal(SEED, 5, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(SEED, 6, B * T * 768).reshape(B, T, 768)
    sess = tsd.Session(unet.model, None, B, L, T, cfg=True)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    ms = []
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
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "freeu": a.freeu, "mode": a.mode if a.freeu else None,
                      "ms_per_step": [round(v, 4) for v in ms], "median": round(float(np.median(ms)), 4)}))


def measure(root, freeu, mode):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)] + \
        (["--freeu", freeu, "--mode", mode] if freeu is not None else [])
    env = {k: val for k, val in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {root} freeu={freeu} mode={mode} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} freeu={freeu} mode={mode} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def pair(on, off):
    r = [x / y for x, y in zip(on, off)]
    d = [1e3 * (x - y) for x, y in zip(on, off)]
    return {"ratio_per_round": [round(v, 5) for v in r], "ratio_median": round(float(np.median(r)), 5), "ratio_range": spread(r),
            "us_per_step_added_per_round": [round(v, 1) for v in d], "us_per_step_added_median": round(float(np.median(d)), 1),
            "us_per_step_added_range": [round(min(d), 1), round(max(d), 1)]}


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    on_arms = [(f"freeu_{c}_{m}", ROOT, c, m) for c in ("diffusers", "channels") for m in ("constant", "modulated")]
    arms = [("parent_1", a.parent_root, None, None), ("parent_2", a.parent_root, None, None), ("freeu_off", ROOT, None, None)] + on_arms
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, root, freeu, mode in arms[k:] + arms[:k]:
            rec[name] = measure(root, freeu, mode)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    rb = [v / parent_median for v in med["freeu_off"]]
    inside = bool(lo <= float(np.median(rb)) <= hi)
    c = {}
    for name, _, conv, mode in on_arms:
        c[name] = pair(med[name], med["freeu_off"])
        c[name]["launches_added"] = (6 if conv == "diffusers" else 10) * (2 if mode == "modulated" else 1)
        c[name]["fp16_bytes_moved_by_the_apply_launches"] = freeu_bytes(conv)
    out = {
        "what": "ms per step(), full-size UNet, B=4 L=64 CFG on, 50 seeded DDPM steps; FreeU arms: b1 1.5, b2 1.6, s1 0.9, s2 0.2 under both "
                "conventions and both modes; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "b_freeu_off_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in rb],
                                           "median": round(float(np.median(rb)), 5), "range": spread(rb), "inside_floor": inside},
        "c_freeu_on_over_off": c,
        "ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_parent_over_parent", "b_freeu_off_over_parent_median", "c_freeu_on_over_off")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
