"""What seeded device-side noise costs a denoise step, that an unseeded session costs what it did, and what the host no longer does:
interleaved same-box pairs at the headline size (B = 8, L = 64, 50 DDPM steps, CFG off).

  python scripts/bench_seeded_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs four fresh processes one after the other, in an order
that rotates from round to round: the parent tree twice, this tree with uploaded noise, this tree seeded.  Each process times P passes of
the 50 enqueued steps with hipEvents on the library's stream (after one warm-up pass) and reports their median; it also takes the host
wall time of what comes before the steps.  Recorded:
  floor the parent against the parent, the A/A spread of this box (the pair noise floor);
  (a) this tree seeded against this tree with uploaded noise - the inline draw against the load of noise[i];
  (b) this tree with uploaded noise against the parent - the unseeded kernels keep their instruction stream;
  (c) before the steps: drawing the [50,8,4,64,64] noise with rng.normal and upload() with it, against upload(noise=None) + set_seeds
      (host wall time, the upload's own synchronise included);
  (d) the ms/step themselves.
Writes FILE (default profiles/seeded_noise_step_pairs.json).  Exits 1 when (b) is outside the floor; (a) is reported with its own flag.

  python scripts/bench_seeded_step.py --worker --root DIR [--seeded]     one measurement, one JSON line (what the driver starts)"""
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
ap.add_argument("--seeded", action="store_true")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=4)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_noise_step_pairs.json"))
a = ap.parse_args()
SEED, B, L, T = 1234, 8, 64, 77


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    unet = tsd.Diffusion(seed=SEED)
    dctx = tsd.default_context()
    nl = B * 4 * L * L
    lat = rng.normal(SEED, 2, nl).reshape(B, 4, L, L)
    ctx = rng.normal(SEED, 5, B * T * 768).reshape(B, T, 768)
    sess = tsd.Session(unet.model, None, B, L, T, cfg=False)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    seeds = list(range(100, 100 + B))
    ms, draw_ms, upload_ms = [], [], []
    noise = None
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        if not a.seeded:
            t0 = time.perf_counter()
            noise = rng.normal(SEED, 3, n * nl).reshape(n, B, 4, L, L)
            draw_ms.append((time.perf_counter() - t0) * 1e3)
        dctx.synchronize()
        t0 = time.perf_counter()
        sess.upload(lat, ctx, None, noise, 7.5)
        if a.seeded:
            sess.set_seeds(seeds)
        dctx.synchronize()
        upload_ms.append((time.perf_counter() - t0) * 1e3)
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    out = sess.latents()
    assert np.isfinite(out).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "seeded": a.seeded, "ms_per_step": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4),
                      "draw_ms": round(float(np.median(draw_ms[1:])), 2) if draw_ms else 0.0,
                      "upload_ms": round(float(np.median(upload_ms[1:])), 2)}))


def measure(root, seeded):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)]
    env = {k: v for k, v in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    r = subprocess.run(cmd + (["--seeded"] if seeded else []), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=300)
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} seeded={seeded} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, False), ("parent_2", a.parent_root, False), ("new_noise", ROOT, False), ("new_seeded", ROOT, True)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        for name, root, seeded in arms[r % 4:] + arms[: r % 4]:
            rec[name] = measure(root, seeded)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {k: [rd[k]["median"] for rd in rounds] for k, _, _ in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    sa = [s / u for s, u in zip(med["new_seeded"], med["new_noise"])]
    b = [n / p for n, p in zip(med["new_noise"], med["parent_1"])]
    sa_med, b_med = float(np.median(sa)), float(np.median(b))
    host = {k: {"draw_ms": float(np.median([rd[k]["draw_ms"] for rd in rounds])),
                "upload_ms": float(np.median([rd[k]["upload_ms"] for rd in rounds]))} for k in ("new_noise", "new_seeded")}
    before_noise = host["new_noise"]["draw_ms"] + host["new_noise"]["upload_ms"]
    before_seeded = host["new_seeded"]["upload_ms"]
    out = {
        "what": "ms per denoise step, B=8 L=64 50 DDPM steps CFG off; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "floor_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "a_new_seeded_over_new_noise": {"per_round": [round(v, 5) for v in sa], "median": round(sa_med, 5),
                                        "inside_floor": bool(lo <= sa_med <= hi),
                                        "ms_per_step_added_median": round(float(np.median(
                                            [s - u for s, u in zip(med["new_seeded"], med["new_noise"])])), 4)},
        "b_new_noise_over_parent": {"per_round": [round(v, 5) for v in b], "median": round(b_med, 5), "inside_floor": bool(lo <= b_med <= hi)},
        "c_host_ms_before_the_steps": {
            "uploaded_noise": {"draw_rng_normal_ms": round(host["new_noise"]["draw_ms"], 2), "upload_ms": round(host["new_noise"]["upload_ms"], 2),
                               "total_ms": round(before_noise, 2)},
            "seeded": {"upload_and_set_seeds_ms": round(before_seeded, 2)},
            "saved_ms_per_call": round(before_noise - before_seeded, 2)},
        "d_ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("floor_parent_over_parent", "a_new_seeded_over_new_noise", "b_new_noise_over_parent",
                                          "c_host_ms_before_the_steps")}))
    sys.exit(0 if out["b_new_noise_over_parent"]["inside_floor"] else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
