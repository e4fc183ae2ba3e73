"""What the torch-norm fused attention kernels (TSD_CHAIN=2) do to a denoise step of a real-checkpoint UNet (kind 6), and that a step at the
default switch costs what it did: interleaved same-box rounds at B = 4, L = 64, CFG on, 50 seeded DDPM steps.

  python scripts/bench_chain_torch_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs four fresh processes one after the other, in an order
that rotates from round to round: the parent tree's step() twice, then this tree's at the default switch and at TSD_CHAIN=2.  Each process
times P passes of the 50 enqueued steps with hipEvents on the library's stream (after one warm-up pass) and reports their median.  Every
process has its own time limit and the first failure ends the run.  Recorded:
  (a) the parent against the parent: the A/A spread of this box (the pair noise floor);
  (b) this tree at the default switch against the parent's median - ACCEPTANCE: the median ratio lies inside (a)'s spread;
  (c) TSD_CHAIN=2 against the default, in ms per step and as a ratio - reported, not gated.
Writes FILE (default profiles/chain_torch_step_pairs.json); exits 1 when (b) is outside the floor.

  python scripts/bench_chain_torch_step.py --worker --root DIR     one measurement, one JSON line (the switch comes from TSD_CHAIN)"""
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
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_torch_step_pairs.json"))
a = ap.parse_args()
SEED, B, L, T = 1234, 4, 64, 77


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    unet = tsd.Diffusion(seed=SEED, variant="diffusion_sd15_torch")
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
    # the launches of one step that ran the fused kernels' class (a head and a tail per C = 320 block at TSD_CHAIN=2, none at the default)
    dctx.profile_begin()
    sess.step(n - 1)
    dctx.synchronize()
    chain = sum(1 for r in dctx.profile_records() if r[0] == "attn_tail_chain")
    dctx.profile_end()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "chain": os.environ.get("TSD_CHAIN"), "chain_launches_per_step": chain,
                      "ms_per_step": [round(v, 4) for v in ms], "median": round(float(np.median(ms)), 4)}))


def measure(root, chain):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)]
    env = {k: val for k, val in os.environ.items() if k not in ("TSD_LIB", "TSD_CHAIN")}  # each tree measures its own library
    if chain:
        env["TSD_CHAIN"] = str(chain)
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {root} chain={chain} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} chain={chain} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, 0), ("parent_2", a.parent_root, 0), ("default", ROOT, 0), ("chain_2", ROOT, 2)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, root, chain in arms[k:] + arms[:k]:
            rec[name] = measure(root, chain)
        assert rec["default"]["chain_launches_per_step"] == 0 and rec["chain_2"]["chain_launches_per_step"] > 0, rec
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    rb = [v / parent_median for v in med["default"]]
    inside = bool(lo <= float(np.median(rb)) <= hi)
    rc = [x / y for x, y in zip(med["chain_2"], med["default"])]
    dc = [x - y for x, y in zip(med["chain_2"], med["default"])]
    out = {
        "what": "ms per step(), full-size torch-norm UNet (kind 6), B=4 L=64 CFG on, 50 seeded DDPM steps; TSD_CHAIN=2: the C = 320 attention "
                "blocks through attn_chain_kernel<KIND_HEAD_T> / <KIND_TAIL_T>; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "b_default_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in rb],
                                         "median": round(float(np.median(rb)), 5), "inside_floor": inside},
        "c_chain_2_over_default": {"ratio_per_round": [round(v, 5) for v in rc], "ratio_median": round(float(np.median(rc)), 5),
                                   "ms_per_step_added_per_round": [round(v, 4) for v in dc], "ms_per_step_added_median": round(float(np.median(dc)), 4)},
        "ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_parent_over_parent", "b_default_over_parent_median", "c_chain_2_over_default")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
