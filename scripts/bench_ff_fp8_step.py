"""What the FP8 feed-forward does to a denoise step of the full-size UNet, and that a step with the option off costs what it did:
interleaved same-box rounds at B = 4, L = 64, CFG on, 50 seeded DDPM steps.

  python scripts/bench_ff_fp8_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs four fresh processes one after the other, in an order
that rotates from round to round: the parent tree's step() twice, then this tree's step() with the option off and on.  Each process times
P passes of the 50 enqueued steps with hipEvents on the library's stream (after one warm-up pass) and reports their median.  Every process
has its own time limit and the first failure ends the run.  Recorded:
  (a) the parent against the parent: the A/A spread of this box (the pair noise floor);
  (b) this tree's step() with the option off against the parent's median - ACCEPTANCE: the median ratio lies inside (a)'s spread;
  (c) option on against option off, in ms per step and as a ratio - reported, not gated;
  (d) per feed-forward shape of that step (M = 2 B H W rows; C = 640 and 1280 - the C = 320 blocks run the fused tail kernel and are left
      alone): the library's own per-launch profile (hipEvents around every launch of ONE step, three more processes): the e4m3 GEMM plus its
      quantiser launch against the fp16 GEMM of the same shape (geglu2's fp16 GEMM from a run with TSD_FOLD_OUT=0, since the default graph
      folds it into the output convolution), and the whole tail: quantise + GEMM + quantise + GEMM + conv_out against geglu1 + the
      folded [h | r] GEMM.  In-situ launches, not a microbenchmark loop: each figure carries its launch's event overhead.
Writes FILE (default profiles/ff_fp8_step_pairs.json); exits 1 when (b) is outside the floor.

  python scripts/bench_ff_fp8_step.py --worker --root DIR [--fp8] [--profile]     one measurement, one JSON line"""
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
ap.add_argument("--fp8", action="store_true", help="worker: turn the option on (this tree's library only)")
ap.add_argument("--profile", action="store_true", help="worker: the per-launch profile of one step instead of the timing")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ff_fp8_step_pairs.json"))
a = ap.parse_args()
SEED, B, L, T = 1234, 4, 64, 77
# (C, divisor of the latent side, blocks) of the attention blocks that run op by op in the full-size UNet
FF_LEVELS = ((640, 2, 5), (1280, 4, 5), (1280, 8, 1))


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    unet = tsd.Diffusion(seed=SEED, variant="diffusion_sd15")
    if a.fp8:  # the parent's library is never asked for what it does not have
        unet.set_ff_fp8(True)
    dctx = tsd.default_context()
    lat = rng.normal(SEED, 4, B * 4 * L * L).reshape(B, 4, L, L).astype(np.float32)
    ctx = rng.normal(SEED, 5, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(SEED, 6, B * T * 768).reshape(B, T, 768)
    sess = tsd.Session(unet.model, None, B, L, T, cfg=True)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    ms, records = [], None
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        sess.upload(lat, ctx, uctx, None, 7.5)
        sess.set_seeds([100 + b for b in range(B)])
        sess.add_noise_seeded(0)
        dctx.synchronize()
        if a.profile and p:
            dctx.profile_begin()
            sess.step(0)
            dctx.synchronize()
            records = [[k, M, N, K, round(t, 5)] for k, M, N, K, _, t in dctx.profile_records()]
            dctx.profile_end()
            break
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    assert np.isfinite(sess.latents()).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "fp8": a.fp8, "records": records, "ms_per_step": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4) if ms else None}))


def measure(root, fp8, profile=False, env_extra=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)] + \
        (["--fp8"] if fp8 else []) + (["--profile"] if profile else [])
    env = {k: val for k, val in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    env.update(env_extra or {})
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {root} fp8={fp8} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} fp8={fp8} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def ff_shapes(off, unfolded, on):
    """(d): per level, ms summed over the level's blocks in ONE step.  A quantiser launch is the record just in front of its GEMM."""
    def gemms(recs, M, N, K):
        return [i for i, r in enumerate(recs) if r[0] == "gemm" and r[1:4] == [M, N, K]]
    out = []
    for C, div, blocks in FF_LEVELS:
        M, Kp1 = 2 * B * (L // div) ** 2, -(-C // 128) * 128
        g1, g2 = gemms(on, M, 8 * C, Kp1), gemms(on, M, C, 4 * C)
        f1, fold, f2 = gemms(off, M, 8 * C, C), gemms(off, M, C, 5 * C), gemms(unfolded, M, C, 4 * C)
        assert len(g1) == len(g2) == len(f1) == len(fold) == len(f2) == blocks, (C, div, len(g1), len(g2), len(f1), len(fold), len(f2))
        assert all(on[i - 1][0] == "elementwise" for i in g1 + g2)
        t = lambda recs, idx, d=0: round(sum(recs[i + d][4] for i in idx), 4)   # noqa: E731
        conv_out = round(sum(on[i + 1][4] for i in g2), 4)   # the fp16 output convolution follows the second e4m3 GEMM
        out.append({"C": C, "M": M, "blocks": blocks,
                    "geglu1": {"fp16_gemm_ms": t(off, f1), "e4m3_gemm_ms": t(on, g1), "quantise_ms": t(on, g1, -1), "N": 8 * C, "K": C},
                    "geglu2": {"fp16_gemm_ms": t(unfolded, f2), "e4m3_gemm_ms": t(on, g2), "quantise_ms": t(on, g2, -1), "N": C, "K": 4 * C},
                    "tail": {"fp16_ms": round(t(off, f1) + t(off, fold), 4),
                             "fp8_ms": round(t(on, g1) + t(on, g1, -1) + t(on, g2) + t(on, g2, -1) + conv_out, 4), "conv_out_ms": conv_out}})
    return out


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, False), ("parent_2", a.parent_root, False), ("fp8_off", ROOT, False), ("fp8_on", ROOT, True)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, root, fp8 in arms[k:] + arms[:k]:
            rec[name] = measure(root, fp8)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    rb = [v / parent_median for v in med["fp8_off"]]
    inside = bool(lo <= float(np.median(rb)) <= hi)
    rc = [x / y for x, y in zip(med["fp8_on"], med["fp8_off"])]
    dc = [x - y for x, y in zip(med["fp8_on"], med["fp8_off"])]
    prof = [measure(ROOT, False, True)["records"], measure(ROOT, False, True, {"TSD_FOLD_OUT": "0"})["records"], measure(ROOT, True, True)["records"]]
    try:
        shapes = ff_shapes(*prof)
    except AssertionError as e:  # the timing stands whatever the profile's records look like
        shapes = {"error": f"the profile's records are not laid out as expected: {e}"}
    out = {
        "what": "ms per step(), full-size UNet, B=4 L=64 CFG on, 50 seeded DDPM steps; option on: the GEGLU linears of the op-by-op attention "
                "blocks on e4m3 operands; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "b_fp8_off_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in rb],
                                         "median": round(float(np.median(rb)), 5), "inside_floor": inside},
        "c_fp8_on_over_off": {"ratio_per_round": [round(v, 5) for v in rc], "ratio_median": round(float(np.median(rc)), 5),
                              "ms_per_step_added_per_round": [round(v, 4) for v in dc], "ms_per_step_added_median": round(float(np.median(dc)), 4)},
        "d_feed_forward_launches_of_one_step": shapes,
        "ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_parent_over_parent", "b_fp8_off_over_parent_median", "c_fp8_on_over_off", "d_feed_forward_launches_of_one_step")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
