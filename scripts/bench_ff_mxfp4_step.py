"""What MXFP4 weights in the 8-bit feed-forward (set_ff_fp8("mxfp4")) do to a denoise step of the full-size UNet, beside the e4m3 weights
and the fp16 path, and that a step with the option off costs what it did: interleaved same-box rounds at B = 4, L = 64, CFG on, 50 seeded
DDPM steps, and the option arms again at B = 1.  Modelled on scripts/bench_ff_fp8_step.py.

  python scripts/bench_ff_mxfp4_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs five fresh processes one after the other, in an order
that rotates from round to round: the parent tree's step() twice, then this tree's step() with the option off, on e4m3 weights (mode 1)
and on MXFP4 weights (mode 2).  Each process times P passes of the 50 enqueued steps with hipEvents on the library's stream (after one
warm-up pass) and reports their median.  Every process has its own time limit and the first failure ends the run.  Recorded:
  (a) the parent against the parent: the A/A spread of this box (the pair noise floor);
  (b) this tree's step() with the option off against the parent's median - ACCEPTANCE: the median ratio lies inside (a)'s spread;
  (c) mode 2 against off and against mode 1, in ms per step and as ratios, at B = 4 and (three arms, same rounds) at B = 1 - reported;
  (d) the six feed-forward GEMM shapes of one B = 4 step (M = 2 B H W rows; C = 640 and 1280 - the C = 320 blocks run the fused tail
      kernel): the library's own per-launch profile, ms summed over the level's blocks, of k_gemm_e4m3_mxfp4 beside k_gemm_e4m3 and the
      fp16 GEMM of the same shape (geglu2's fp16 GEMM from a run with TSD_FOLD_OUT=0, since the default graph folds it into the output
      convolution).  In-situ launches, not a microbenchmark loop: each figure carries its launch's event overhead.
Writes FILE (default profiles/ff_mxfp4_step_pairs.json); exits 1 when (b) is outside the floor.

  python scripts/bench_ff_mxfp4_step.py --worker --root DIR [--mode 0|1|2] [--batch B] [--profile]     one measurement, one JSON line"""
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
ap.add_argument("--mode", type=int, default=0, help="worker: 0 off, 1 e4m3 weights, 2 MXFP4 weights (this tree's library only)")
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--profile", action="store_true", help="worker: the per-launch profile of one step instead of the timing")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ff_mxfp4_step_pairs.json"))
a = ap.parse_args()
SEED, L, T = 1234, 64, 77
# (C, divisor of the latent side, blocks) of the attention blocks that run op by op in the full-size UNet
FF_LEVELS = ((640, 2, 5), (1280, 4, 5), (1280, 8, 1))


def worker():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    from tsd import rng
    tsd.set_strict(True)
    B = a.batch
    unet = tsd.Diffusion(seed=SEED, variant="diffusion_sd15")
    if a.mode:  # the parent's library is never asked for what it does not have
        unet.set_ff_fp8("mxfp4" if a.mode == 2 else True)
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
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "mode": a.mode, "batch": B, "records": records, "ms_per_step": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4) if ms else None}))


def measure(root, mode, batch=4, profile=False, env_extra=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps),
           "--mode", str(mode), "--batch", str(batch)] + (["--profile"] if profile else [])
    env = {k: val for k, val in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    env.update(env_extra or {})
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {root} mode={mode} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} mode={mode} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def ff_shapes(off, unfolded, e4m3, mx, B):
    """(d): per level and linear, ms summed over the level's blocks in ONE step, the three GEMMs of the same shape side by side."""
    def gemm_ms(recs, M, N, K, blocks):
        t = [r[4] for r in recs if r[0] == "gemm" and r[1:4] == [M, N, K]]
        assert len(t) == blocks, (M, N, K, len(t), blocks)
        return round(sum(t), 4)
    out = []
    for C, div, blocks in FF_LEVELS:
        M, Kp1 = 2 * B * (L // div) ** 2, -(-C // 128) * 128
        for name, N, K, Kp, f16 in (("geglu1", 8 * C, C, Kp1, off), ("geglu2", C, 4 * C, 4 * C, unfolded)):
            out.append({"linear": name, "C": C, "M": M, "N": N, "K": K, "blocks": blocks, "fp16_gemm_ms": gemm_ms(f16, M, N, K, blocks),
                        "e4m3_gemm_ms": gemm_ms(e4m3, M, N, Kp, blocks), "mxfp4_gemm_ms": gemm_ms(mx, M, N, Kp, blocks)})
    return out


def ratios(x, y):
    r, d = [p / q for p, q in zip(x, y)], [p - q for p, q in zip(x, y)]
    return {"ratio_per_round": [round(v, 5) for v in r], "ratio_median": round(float(np.median(r)), 5),
            "ms_per_step_added_median": round(float(np.median(d)), 4)}


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, 0), ("parent_2", a.parent_root, 0), ("off", ROOT, 0), ("e4m3", ROOT, 1), ("mxfp4", ROOT, 2)]
    rounds, rounds1 = [], []
    t0 = time.time()
    for r in range(a.rounds):
        rec, k = {}, r % len(arms)
        for name, root, mode in arms[k:] + arms[:k]:
            rec[name] = measure(root, mode)
        rounds.append(rec)
        rec1, k1 = {}, r % 3
        for name, root, mode in arms[2 + k1:] + arms[2:2 + k1]:   # B = 1: this tree's three arms
            rec1[name] = measure(root, mode, batch=1)
        rounds1.append(rec1)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())) + "  | B=1 " +
              "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec1.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    med1 = {arm[0]: [rd[arm[0]]["median"] for rd in rounds1] for arm in arms[2:]}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    rb = [v / parent_median for v in med["off"]]
    inside = bool(lo <= float(np.median(rb)) <= hi)
    prof = [measure(ROOT, 0, profile=True)["records"], measure(ROOT, 0, profile=True, env_extra={"TSD_FOLD_OUT": "0"})["records"],
            measure(ROOT, 1, profile=True)["records"], measure(ROOT, 2, profile=True)["records"]]
    try:
        shapes = ff_shapes(*prof, 4)
    except AssertionError as e:  # the timing stands whatever the profile's records look like
        shapes = {"error": f"the profile's records are not laid out as expected: {e}"}
    out = {
        "what": "ms per step(), full-size UNet, L=64 CFG on, 50 seeded DDPM steps; mode 1: the GEGLU linears of the op-by-op attention blocks "
                "on e4m3 operands; mode 2: the same with MXFP4 weights; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "b_off_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in rb],
                                     "median": round(float(np.median(rb)), 5), "inside_floor": inside},
        "c_B4": {"mxfp4_over_off": ratios(med["mxfp4"], med["off"]), "mxfp4_over_e4m3": ratios(med["mxfp4"], med["e4m3"]),
                 "e4m3_over_off": ratios(med["e4m3"], med["off"])},
        "c_B1": {"mxfp4_over_off": ratios(med1["mxfp4"], med1["off"]), "mxfp4_over_e4m3": ratios(med1["mxfp4"], med1["e4m3"]),
                 "e4m3_over_off": ratios(med1["e4m3"], med1["off"])},
        "d_feed_forward_gemms_of_one_B4_step": shapes,
        "ms_per_step": {"B4": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
                        "B1": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med1.items()}},
        "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_parent_over_parent", "b_off_over_parent_median", "c_B4", "c_B1", "d_feed_forward_gemms_of_one_B4_step")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
