"""What v-prediction costs a denoise step, and that a default (epsilon) step costs what it did: interleaved same-box rounds at B = 8,
L = 64, CFG on, 50 seeded DDPM steps.

  python scripts/bench_vpred_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs six fresh processes one after the other, in an order that
rotates from round to round: the parent tree's step() twice, this tree's step() with the defaults and with set_prediction("v", True),
this tree's advance() with eight slots likewise.  Each process times P passes of the 50 enqueued steps with hipEvents on the library's
stream (after one warm-up pass) and reports their median.  Every process has its own time limit and the first failure ends the run.
The v arms run the same sampler on the same timestep list: under v the DDPM step is k_sampler_step_v_seeded where the default is
k_ddpm_step_seeded, the same bytes read and written and the same number of launches.  Recorded:
  floor the parent against the parent, the A/A spread of this box (the pair noise floor);
  (a) this tree's default step() against the parent's step() - ACCEPTANCE: the median ratio lies inside the floor;
  (b) step() under v against the default step(), same tree - reported, not gated, as a ratio and in us per step;
  (c) advance() with eight slots under v against eight default ones, same tree - reported likewise.
Writes FILE (default profiles/vpred_step_pairs.json); exits 1 when (a) is outside the floor.

  python scripts/bench_vpred_step.py --worker --root DIR [--slots] [--v]     one measurement, one JSON line"""
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
ap.add_argument("--slots", action="store_true")
ap.add_argument("--v", action="store_true")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=4)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vpred_step_pairs.json"))
a = ap.parse_args()
SEED, B, L, T = 1234, 8, 64, 77


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    unet = tsd.Diffusion(seed=SEED)
    dctx = tsd.default_context()
    lat = rng.normal(SEED, 4, B * 4 * L * L).reshape(B, 4, L, L).astype(np.float32)
    ctx = rng.normal(SEED, 5, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(SEED, 6, B * T * 768).reshape(B, T, 768)
    sess = tsd.Session(unet.model, None, B, L, T, cfg=True)
    if a.v:  # the parent's library is never asked for what it does not have
        sess.set_prediction("v", True)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    if a.slots:
        sess.slots_open()
    ms = []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        if a.slots:
            for b in range(B):
                sess.slot_start(b, ctx[b], uctx[b], latents=lat[b], noise_at_start=True, seed=100 + b, start_index=0, cfg_scale=7.5)
        else:
            sess.upload(lat, ctx, uctx, None, 7.5)
            sess.set_seeds([100 + b for b in range(B)])
            sess.add_noise_seeded(0)
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.advance() if a.slots else sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    out = np.stack([sess.slot_latents(b) for b in range(B)]) if a.slots else sess.latents()
    assert np.isfinite(out).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "slots": a.slots, "v": a.v, "ms_per_step": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4)}))


def measure(root, slots, v):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)] + \
        (["--slots"] if slots else []) + (["--v"] if v else [])
    env = {k: val for k, val in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {root} slots={slots} v={v} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} slots={slots} v={v} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def pair(on, off, lo, hi):
    r = [x / y for x, y in zip(on, off)]
    return {"per_round": [round(v, 5) for v in r], "median": round(float(np.median(r)), 5), "range": spread(r),
            "inside_floor": bool(lo <= float(np.median(r)) <= hi),
            "us_per_step_added_median": round(1e3 * float(np.median([x - y for x, y in zip(on, off)])), 2)}


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, False, False), ("parent_2", a.parent_root, False, False), ("step_eps", ROOT, False, False),
            ("step_v", ROOT, False, True), ("advance_eps", ROOT, True, False), ("advance_v", ROOT, True, True)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, root, slots, v in arms[k:] + arms[:k]:
            rec[name] = measure(root, slots, v)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    ra = [v / parent_median for v in med["step_eps"]]
    inside = bool(lo <= float(np.median(ra)) <= hi)
    out = {
        "what": "ms per step() / advance(), B=8 L=64 CFG on, 50 seeded DDPM steps (advance: eight img2img slots from index 0); v arms: "
                "set_prediction('v', zero_terminal_snr=True); interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "floor_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "a_step_default_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in ra],
                                              "median": round(float(np.median(ra)), 5), "range": spread(ra), "inside_floor": inside},
        "b_step_v_over_eps": pair(med["step_v"], med["step_eps"], lo, hi),
        "c_advance_v_over_eps": pair(med["advance_v"], med["advance_eps"], lo, hi),
        "d_ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("floor_parent_over_parent", "a_step_default_over_parent_median", "b_step_v_over_eps",
                                          "c_advance_v_over_eps")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
