"""What the CLIP vision encoder costs: `tsd_clip_vision_forward` (host in, host out, synchronous) in ms per call at B = 1, 4, 16 for
224x224 and 512x512 inputs, and the achieved TF/s by `tsd_flop_count`.  Report only: no threshold.

  python scripts/bench_clip_vision.py [--rounds R] [--iters N] [--out FILE]

Every measurement runs in a fresh process (its own context, model and plan); the rounds visit the six cases in an order that rotates from
round to round; a worker times N calls after two warm-up calls (the first builds the coefficient tables and the workspace plan) with the
host clock around the synchronous entry and reports their median.  Every process has its own time limit and the first failure ends the
run.  Recorded per case: the median and the range over the rounds, and TF/s = B * tsd_flop_count(kind) / median.  The call includes the
host-to-device copy of the pixels (B * 3 * H * W floats) and the copy back of B * 1024 floats.
Writes FILE (default profiles/clip_vision_forward.json).

  python scripts/bench_clip_vision.py --worker --B B --side S     one measurement, one JSON line"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--worker", action="store_true")
ap.add_argument("--B", type=int, default=1)
ap.add_argument("--side", type=int, default=224)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--worker-timeout", type=int, default=120)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vision_forward.json"))
a = ap.parse_args()
CASES = [(B, side) for side in (224, 512) for B in (1, 4, 16)]


def worker():
    sys.path.insert(0, os.path.join(ROOT, "stable-diffusion.mojo_amd"))
    import tsd
    tsd.set_strict(True)
    enc = tsd.CLIPVision(seed=1234)
    img = np.random.default_rng(a.B * 1000 + a.side).uniform(0.0, 255.0, size=(a.B, 3, a.side, a.side)).astype(np.float32)
    for _ in range(2):
        out = enc.forward(img)
    assert np.isfinite(out).all()
    ms = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        enc.forward(img)
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"B": a.B, "side": a.side, "ms": statistics.median(ms), "ms_min": min(ms), "gflop_per_image": tsd.flop_count("clip_vision_h", 0, 0)}), flush=True)


def main():
    runs = {c: [] for c in CASES}
    gf = None
    for r in range(a.rounds):
        order = CASES[r % len(CASES):] + CASES[:r % len(CASES)]
        for B, side in order:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--B", str(B), "--side", str(side), "--iters", str(a.iters)],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                sys.exit(f"worker B={B} side={side} ended with status {p.returncode}: nothing more is started")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            gf = rec["gflop_per_image"]
            runs[(B, side)].append(rec["ms"])
            print(f"round {r} B={B} {side}x{side}: {rec['ms']:.3f} ms", flush=True)
    out = {"what": "tsd_clip_vision_forward, ms per synchronous host-in / host-out call (scripts/bench_clip_vision.py)", "rounds": a.rounds, "iters": a.iters,
           "gflop_per_image": gf, "cases": []}
    for (B, side), ms in runs.items():
        med = statistics.median(ms)
        out["cases"].append({"B": B, "H": side, "W": side, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "ms_rounds": ms,
                             "tflops": B * gf / med})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for c in out["cases"]:
        print(f"B={c['B']:2d} {c['H']}x{c['W']}: {c['ms_median']:.3f} ms [{c['ms_min']:.3f}, {c['ms_max']:.3f}]  {c['tflops']:.1f} TF/s")


if __name__ == "__main__":
    worker() if a.worker else main()
