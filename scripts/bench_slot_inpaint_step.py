"""What inpainting slots cost a denoise tick, and that an advance without them costs what it did: interleaved same-box rounds at B = 8,
L = 64, CFG on, 50 seeded DDPM steps.

  python scripts/bench_slot_inpaint_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs four fresh processes one after the other, in an order
that rotates from round to round: the parent tree's advance() twice, this tree's advance() with no inpainting slot (k_slot_update, as
before), this tree's advance() with all eight slots inpainting (k_slot_update_blend).  All eight slots are img2img requests from index 0,
started together.  Each process times P passes of the 50 enqueued ticks with hipEvents on the library's stream (after one warm-up pass)
and reports their median.  Every process has its own time limit and the first failure ends the run.  Recorded:
  floor the parent against the parent, the A/A spread of this box (the pair noise floor);
  (a) this tree's advance() without inpainting against the parent's advance() - ACCEPTANCE: the median ratio lies inside the floor;
  (b) advance() with eight inpainting slots against advance() with none, same tree - reported, not gated (the lockstep blend launch cost
      +4.2 us per step, profiles/inpaint_step_pairs.json; fused into the update the expectation is less);
  (c) slot_set_inpaint of one slot, host wall time with its own synchronise.
Writes FILE (default profiles/slot_inpaint_step_pairs.json); exits 1 when (a) is outside the floor.

  python scripts/bench_slot_inpaint_step.py --worker --root DIR [--inpaint]     one measurement, one JSON line (what the driver starts)"""
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
ap.add_argument("--inpaint", action="store_true")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=4)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slot_inpaint_step_pairs.json"))
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
    # a mask per slot with 0, 1 and fractions: every branch of the blend's arithmetic sees data
    cell = np.arange(L * L).reshape(L, L)
    masks = [np.clip(((cell * (2 * b + 3) + b) % 13 - 3) / 8.0, 0.0, 1.0).astype(np.float32) for b in range(B)]
    sess = tsd.Session(unet.model, None, B, L, T, cfg=True)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    sess.slots_open()
    ms, set_ms = [], []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        for b in range(B):
            sess.slot_start(b, ctx[b], uctx[b], latents=lat[b], noise_at_start=True, seed=100 + b, start_index=0, cfg_scale=7.5)
            if a.inpaint:
                dctx.synchronize()
                t0 = time.perf_counter()
                sess.slot_set_inpaint(b, masks[b], lat[b])
                if p:
                    set_ms.append((time.perf_counter() - t0) * 1e3)
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.advance()
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    out = np.stack([sess.slot_latents(b) for b in range(B)])
    assert np.isfinite(out).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "inpaint": a.inpaint, "ms_per_tick": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4), "slot_set_inpaint_ms": [round(v, 3) for v in set_ms]}))


def measure(root, inpaint):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)]
    env = {k: v for k, v in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    try:
        r = subprocess.run(cmd + (["--inpaint"] if inpaint else []), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {root} inpaint={inpaint} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} inpaint={inpaint} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, False), ("parent_2", a.parent_root, False), ("new_plain", ROOT, False), ("new_inpaint", ROOT, True)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        for name, root, ip in arms[r % 4:] + arms[: r % 4]:
            rec[name] = measure(root, ip)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {k: [rd[k]["median"] for rd in rounds] for k, _, _ in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    ra = [v / parent_median for v in med["new_plain"]]
    rb = [i / p for i, p in zip(med["new_inpaint"], med["new_plain"])]
    sets = [v for rd in rounds for v in rd["new_inpaint"]["slot_set_inpaint_ms"]]
    inside = bool(lo <= float(np.median(ra)) <= hi)
    out = {
        "what": "ms per advance(), B=8 L=64 CFG on, 50 seeded DDPM steps, eight img2img slots from index 0; interleaved same-box rounds, "
                "one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "floor_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "a_new_plain_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in ra],
                                           "median": round(float(np.median(ra)), 5), "range": spread(ra), "inside_floor": inside},
        "b_new_inpaint_over_new_plain": {"per_round": [round(v, 5) for v in rb], "median": round(float(np.median(rb)), 5), "range": spread(rb),
                                         "inside_floor": bool(lo <= float(np.median(rb)) <= hi),
                                         "us_per_tick_added_median": round(1e3 * float(np.median(
                                             [i - p for i, p in zip(med["new_inpaint"], med["new_plain"])])), 2),
                                         "lockstep_blend_launch_us_per_step": 4.2},
        "c_slot_set_inpaint_ms": {"n": len(sets), "median": round(float(np.median(sets)), 3), "range": spread(sets),
                                  "what": "host wall time of one slot_set_inpaint (two copies, the noise fill, its own synchronise)"},
        "d_ms_per_tick": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("floor_parent_over_parent", "a_new_plain_over_parent_median", "b_new_inpaint_over_new_plain",
                                          "c_slot_set_inpaint_ms")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
