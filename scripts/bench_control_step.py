"""What a ControlNet costs a denoise step of the full-size UNet, and that an uncontrolled step costs what it did: interleaved same-box
rounds at B = 4, L = 64, CFG on, 50 seeded DDPM steps.

  python scripts/bench_control_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs six fresh processes one after the other, in an order that
rotates from round to round: the parent tree's step() twice, then this tree's step() without control, with control (scale 1 on both CFG
halves), with control at scale exactly 0, and with control under TSD_CONTROL_STATS=0.  Each process times P passes of the 50 enqueued
steps with hipEvents on the library's stream (after one warm-up pass) and reports their median.  Every process has its own time limit and
the first failure ends the run.  Recorded:
  (a) the parent against the parent, the A/A spread of this box (the pair noise floor);
  (b) this tree's uncontrolled step() against the parent's median - ACCEPTANCE: the median ratio lies inside (a)'s spread (the refactored
      full-size loop may cost nothing);
  (c) the controlled step() against the uncontrolled one, in ms and as a ratio - reported, not gated (the ControlNet is 21 of the UNet's
      45 steps, the expensive-resolution ones, plus the hint features' add, thirteen 1x1 convolutions and the injection);
  (d) the injection launch: a sample at scale exactly 0 is skipped by every workgroup of k_control_inject before its first load, so the
      controlled step at scale 0 is the controlled step minus the injection's work (the empty launch stays).  The difference against
      (c)'s controlled arm, in us, and against the bytes the launch moves at this shape - x and r read, y written, fp16 - as a fraction
      of the 8 TB/s HBM peak, to set beside k_gn_apply's figure in profiles/.  At scale 0 the decoder blocks read the producers'
      statistics, at scale 1 the injection's: the same branches either way;
  (e) the controlled step() with the injection's statistics discarded (every consumer runs its own statistics pass) against (c): what
      the hand-over buys.
Writes FILE (default profiles/control_step_pairs.json); exits 1 when (b) is outside the floor.

  python scripts/bench_control_step.py --worker --root DIR [--control SCALE]     one measurement, one JSON line"""
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
ap.add_argument("--control", type=float, default=None, help="worker: set_control with this scale (absent: no control)")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_step_pairs.json"))
a = ap.parse_args()
SEED, B, L, T = 1234, 4, 64, 77
HBM_PEAK_GBS = 8000.0
# (C, divisor of the latent side) of the thirteen tensors the injection rewrites
INJECTED = ((320, 1), (320, 1), (320, 1), (320, 2), (640, 2), (640, 2), (640, 4), (1280, 4), (1280, 4), (1280, 8), (1280, 8), (1280, 8), (1280, 8))


def injection_bytes():
    """x read, r read, y written, fp16, at the UNet's batch 2B."""
    return 3 * 2 * sum(2 * B * (L // d) * (L // d) * c for c, d in INJECTED)


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
    cn = hint = None
    if a.control is not None:  # the parent's library is never asked for what it does not have
        cn = tsd.ControlNet(seed=SEED)   # timing only: the zero convolutions may stay at zero
        hint = rng.uniform(SEED, 7, B * 3 * 64 * L * L, 0.5).reshape(B, 3, 8 * L, 8 * L) + np.float32(0.5)
    ms = []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        sess.upload(lat, ctx, uctx, None, 7.5)
        sess.set_seeds([100 + b for b in range(B)])
        sess.add_noise_seeded(0)
        if cn is not None and p == 0:
            sess.set_control(cn, hint, scale=a.control)   # it outlives the later uploads
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    assert np.isfinite(sess.latents()).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "control": a.control, "stats": os.environ.get("TSD_CONTROL_STATS", "1"),
                      "ms_per_step": [round(v, 4) for v in ms], "median": round(float(np.median(ms)), 4)}))


def measure(root, control, stats):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)] + \
        (["--control", repr(control)] if control is not None else [])
    env = {k: val for k, val in os.environ.items() if k not in ("TSD_LIB", "TSD_CONTROL_STATS")}  # each tree measures its own library
    if not stats:
        env["TSD_CONTROL_STATS"] = "0"
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {root} control={control} stats={stats} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} control={control} stats={stats} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def pair(on, off):
    r = [x / y for x, y in zip(on, off)]
    d = [x - y for x, y in zip(on, off)]
    return {"per_round": [round(v, 5) for v in r], "median": round(float(np.median(r)), 5), "range": spread(r),
            "ms_per_step_added_median": round(float(np.median(d)), 4), "ms_per_step_added_range": spread(d)}


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, None, True), ("parent_2", a.parent_root, None, True), ("step_plain", ROOT, None, True),
            ("step_control", ROOT, 1.0, True), ("step_control_scale0", ROOT, 0.0, True), ("step_control_nostats", ROOT, 1.0, False)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, root, control, stats in arms[k:] + arms[:k]:
            rec[name] = measure(root, control, stats)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    rb = [v / parent_median for v in med["step_plain"]]
    inside = bool(lo <= float(np.median(rb)) <= hi)
    inj_us = [1e3 * (x - y) for x, y in zip(med["step_control"], med["step_control_scale0"])]
    inj_med = float(np.median(inj_us))
    nbytes = injection_bytes()
    out = {
        "what": "ms per step(), full-size UNet, B=4 L=64 CFG on, 50 seeded DDPM steps; control arms: set_control(scale 1 / scale 0 / scale 1 "
                "under TSD_CONTROL_STATS=0); interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "b_step_plain_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in rb],
                                            "median": round(float(np.median(rb)), 5), "range": spread(rb), "inside_floor": inside},
        "c_step_control_over_plain": pair(med["step_control"], med["step_plain"]),
        "d_injection": {"us_per_step_per_round": [round(v, 2) for v in inj_us], "us_per_step_median": round(inj_med, 2), "bytes_moved": nbytes,
                        "gb_per_s": round(nbytes / (inj_med * 1e-6) / 1e9, 1) if inj_med > 0 else None,
                        "fraction_of_hbm_peak": round(nbytes / (inj_med * 1e-6) / 1e9 / HBM_PEAK_GBS, 4) if inj_med > 0 else None,
                        "how": "controlled step at scale 1 minus controlled step at scale exactly 0 (every workgroup of the launch returns before its first load)"},
        "e_step_control_nostats_over_control": pair(med["step_control_nostats"], med["step_control"]),
        "ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_parent_over_parent", "b_step_plain_over_parent_median", "c_step_control_over_plain", "d_injection",
                                          "e_step_control_nostats_over_control")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
