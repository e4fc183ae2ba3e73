"""What slot mode costs a denoise tick, that a lockstep session costs what it did, and what starting one slot costs: interleaved same-box
rounds at B = 8, L = 64, CFG on, 50 seeded DDPM steps.

  python scripts/bench_slot_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs four fresh processes one after the other, in an order
that rotates from round to round: the parent tree's step() twice, this tree's step(), this tree's advance() with all eight slots started
together.  Each process times P passes of the 50 enqueued ticks with hipEvents on the library's stream (after one warm-up pass) and
reports their median.  Recorded:
  floor the parent against the parent, the A/A spread of this box (the pair noise floor);
  (a) this tree's step() against the parent's step() - the sampler launch is unchanged;
  (b) this tree's advance() against the parent's step() - one more small elementwise launch (the time-row gather) and the per-slot
      update kernel in place of the lockstep one;
  (c) slot_start of one slot, host wall time with its own synchronise, hoist on (context conversion, that sample's K / V^T, latents);
  occupancy of SlotScheduler on a fixed mixed queue (host arithmetic on a counting session: active slot-ticks over B * advances).
Writes FILE (default profiles/slot_step_pairs.json).  No threshold: the ratios and their ranges are the result.

  python scripts/bench_slot_step.py --worker --root DIR [--advance]     one measurement, one JSON line (what the driver starts)"""
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
ap.add_argument("--advance", action="store_true")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=4)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slot_step_pairs.json"))
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
    lat = np.zeros((B, 4, L, L), dtype=np.float32)
    ctx = rng.normal(SEED, 5, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(SEED, 6, B * T * 768).reshape(B, T, 768)
    seeds = list(range(100, 100 + B))
    sess = tsd.Session(unet.model, None, B, L, T, cfg=True)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    ms, start_ms = [], []
    if a.advance:
        sess.slots_open()
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        if a.advance:
            for b in range(B):
                dctx.synchronize()
                t0 = time.perf_counter()
                sess.slot_start(b, ctx[b], uctx[b], seed=seeds[b], cfg_scale=7.5)
                if p:
                    start_ms.append((time.perf_counter() - t0) * 1e3)
        else:
            sess.upload(lat, ctx, uctx, None, 7.5)
            sess.set_seeds(seeds)
            sess.seed_latents()
        dctx.synchronize()
        dctx.timer_start()
        if a.advance:
            for i in range(n):
                sess.advance()
        else:
            for i in range(n):
                sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    out = np.stack([sess.slot_latents(b) for b in range(B)]) if a.advance else sess.latents()
    assert np.isfinite(out).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "advance": a.advance, "ms_per_step": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4),
                      "slot_start_ms": [round(v, 3) for v in start_ms], "nl": nl}))


def measure(root, advance):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)]
    env = {k: v for k, v in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    r = subprocess.run(cmd + (["--advance"] if advance else []), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=300)
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} advance={advance} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


class CountingSession:
    """The slot methods on the host alone: what SlotScheduler's occupancy needs."""

    def __init__(self, nb, num_steps):
        self.B, self.num_steps, self.index = nb, num_steps, [None] * nb

    def slot_start(self, b, context, uncond_context=None, latents=None, noise_at_start=False, seed=0, start_index=0, cfg_scale=7.5):
        self.index[b] = start_index

    def advance(self):
        done = []
        for b, i in enumerate(self.index):
            if i is not None:
                self.index[b] = i + 1 if i + 1 < self.num_steps else None
                if self.index[b] is None:
                    done.append(b)
        return done

    def slot_latents(self, b):
        return None


def occupancy():
    """A fixed mixed queue: 40 requests, every fourth txt2img, the others img2img of strength 0.3 / 0.5 / 0.8 in turn."""
    sys.path.insert(0, os.path.join(ROOT, "stable-diffusion.mojo_amd"))
    from tsd.serve import Request, SlotScheduler
    strengths = [None, 0.3, 0.5, 0.8]
    lat = np.zeros((4, 1, 1), dtype=np.float32)
    queue = [Request(k, None, None, k, 7.5, None if strengths[k % 4] is None else lat, strengths[k % 4]) for k in range(40)]
    sched = SlotScheduler(CountingSession(B, a.steps), iter(queue))
    n = sum(1 for _ in sched)
    lockstep = a.steps * -(-len(queue) // B)  # ceil(40 / 8) lockstep batches of 50 steps, every sample the full schedule
    return {"queue": "40 requests: k % 4 == 0 txt2img, else img2img of strength 0.3 / 0.5 / 0.8 in turn; B = 8, 50 steps",
            "yielded": n, "advances": sched.advances, "active_slot_ticks": sched.active_ticks, "occupancy": round(sched.occupancy, 4),
            "lockstep_ticks_if_each_batch_ran_the_full_schedule": lockstep}


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, False), ("parent_2", a.parent_root, False), ("new_step", ROOT, False), ("new_advance", ROOT, True)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        for name, root, adv in arms[r % 4:] + arms[: r % 4]:
            rec[name] = measure(root, adv)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {k: [rd[k]["median"] for rd in rounds] for k, _, _ in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    ra = [s / p for s, p in zip(med["new_step"], med["parent_1"])]
    rb = [s / p for s, p in zip(med["new_advance"], med["parent_1"])]
    starts = [v for rd in rounds for v in rd["new_advance"]["slot_start_ms"]]
    out = {
        "what": "ms per denoise tick, B=8 L=64 CFG on, 50 seeded DDPM steps; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "floor_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "a_new_step_over_parent_step": {"per_round": [round(v, 5) for v in ra], "median": round(float(np.median(ra)), 5),
                                        "range": spread(ra), "inside_floor": bool(lo <= float(np.median(ra)) <= hi)},
        "b_new_advance_over_parent_step": {"per_round": [round(v, 5) for v in rb], "median": round(float(np.median(rb)), 5),
                                           "range": spread(rb), "inside_floor": bool(lo <= float(np.median(rb)) <= hi),
                                           "ms_per_tick_added_median": round(float(np.median(
                                               [s - p for s, p in zip(med["new_advance"], med["parent_1"])])), 4)},
        "c_slot_start_ms": {"n": len(starts), "median": round(float(np.median(starts)), 3), "range": spread(starts),
                            "what": "host wall time of one slot_start (its own synchronise included), hoist on, txt2img request"},
        "d_ms_per_tick": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "scheduler_occupancy": occupancy(),
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("floor_parent_over_parent", "a_new_step_over_parent_step", "b_new_advance_over_parent_step",
                                          "c_slot_start_ms", "scheduler_occupancy")}))


if __name__ == "__main__":
    worker() if a.worker else driver()
