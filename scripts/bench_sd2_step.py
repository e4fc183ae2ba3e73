"""What the SD-2.x kinds cost and that the old kinds cost what they did: interleaved same-box rounds, one fresh process per measurement.

  python scripts/bench_sd2_step.py --parent-root DIR [--nocheck-lib FILE] [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  FILE is this tree's library built with -DTSD_ATTN_CHECK_EVERY=1000000
(`make BUILD=build_nocheck OUT=../lib/libtsd_nocheck.so EXTRA=-DTSD_ATTN_CHECK_EVERY=1000000`): the d = 64 kernel without its early
look.  Every round runs its processes one after the other in an order that rotates from round to round; every process has its own time
limit and the first failure ends the run.  Recorded:
  (1) the kind-6 step() at B = 4, L = 64, CFG on, 50 seeded DDPM steps: the parent against the parent (the A/A spread of this box) and
      this tree against the parent's median - "old kinds unchanged" holds when the median ratio lies inside that spread;
  (2) the SD-2 step() at the same shape beside kind 6's, with the per-class times of one profiled pass (tsd_ctx_profile_end);
  (3) tsd_debug_attn_bench at (d, H, Sq, Sk) = (64, 5, 4096, 4096), (64, 10, 1024, 1024), (64, 20, 256, 256), (64, 5, 4096, 77) beside the
      equal-FLOP d = 40 / 80 / 160 calls at H = 8 (B = 8);
  (4) the (64, 5, 4096, 4096) launch (B = 2) with every workgroup repeating (a key of tile 4 of 64 is 30 log2 units up) against the same
      launch with none repeating, on this tree's library and on the one without the early look: kernel time from the profiler's
      flash_attention class around tsd_debug_attn_run.
Writes FILE (default profiles/sd2_step_pairs.json); exits 1 when (1) is outside the floor.

  python scripts/bench_sd2_step.py --worker step|attn|peaked --root DIR [--variant V] [--lib FILE]     one measurement, one JSON line"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--worker", choices=("step", "attn", "peaked"))
ap.add_argument("--root", default=ROOT)
ap.add_argument("--variant", default="diffusion_sd15_torch")
ap.add_argument("--lib", default=None, help="another build of this tree's library (TSD_LIB)")
ap.add_argument("--parent-root")
ap.add_argument("--nocheck-lib", default=os.path.join(ROOT, "stable-diffusion.mojo_amd", "lib", "libtsd_nocheck.so"))
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sd2_step_pairs.json"))
a = ap.parse_args()
SEED, B, L, T = 1234, 4, 64, 77
ATTN_CALLS = [(64, 5, 4096, 4096), (40, 8, 4096, 4096), (64, 10, 1024, 1024), (80, 8, 1024, 1024), (64, 20, 256, 256), (160, 8, 256, 256),
              (64, 5, 4096, 77), (40, 8, 4096, 77)]


def _tsd():
    sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
    import tsd
    tsd.set_strict(True)
    return tsd


def worker_step():
    tsd = _tsd()
    from tsd import rng
    unet = tsd.Diffusion(seed=SEED, variant=a.variant)
    W = 1024 if a.variant == "diffusion_sd2" else 768
    dctx = tsd.default_context()
    lat = rng.normal(SEED, 4, B * 4 * L * L).reshape(B, 4, L, L).astype(np.float32)
    ctx = rng.normal(SEED, 5, B * T * W).reshape(B, T, W)
    uctx = rng.normal(SEED, 6, B * T * W).reshape(B, T, W)
    sess = tsd.Session(unet.model, None, B, L, T, cfg=True)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    ms, classes = [], None
    for p in range(a.passes + 2):  # pass 0 warms every shape up; the last pass is the profiled one (not timed)
        sess.upload(lat, ctx, uctx, None, 7.5)
        sess.set_seeds([100 + b for b in range(B)])
        sess.add_noise_seeded(0)
        dctx.synchronize()
        if p == a.passes + 1:
            dctx.profile_begin()
            for i in range(n):
                sess.step(i)
            classes = {k: [round(v[0] / n, 4), v[1] // n] for k, v in dctx.profile_end().items() if v[1]}
            continue
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    assert np.isfinite(sess.latents()).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "variant": a.variant, "ms_per_step": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4), "class_ms_per_step_and_launches": classes}))


def worker_attn():
    tsd = _tsd()
    from tsd._lib import lib
    ctx = tsd.default_context()
    ms = C.c_float()
    out = {}
    for d, H, Sq, Sk in ATTN_CALLS:
        rc = lib().tsd_debug_attn_bench(ctx.h, 8, H, d, Sq, Sk, 20, C.byref(ms))
        assert rc == 0, tsd._lib.last_error()
        fl = 4.0 * 8 * H * Sq * Sk * d
        out[f"d{d}_h{H}_{Sq}x{Sk}"] = {"us": round(ms.value * 1e3, 2), "tflops": round(fl / (ms.value * 1e-3) / 1e12, 1)}
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "calls": out}))


def worker_peaked():
    tsd = _tsd()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import attn64_ref as R
    import attn_ref as A
    import replay
    ctx = tsd.default_context()
    d = R.attn_desc(2, 5, 4096, 4096, dense=True)
    out = {}
    for name, kind in (("none_repeat", "flat"), ("all_repeat", "spike_t4of64")):
        ops = R.make_inputs(d, kind, seed=3)
        best, reps = [], None
        for it in range(6):
            ctx.profile_begin()
            rc, _, info = replay.run("tsd_debug_attn_run", ctx, d, ops, A.AO, A.INPUTS, ("O",), A.dtype_of, A.extents)
            prof = ctx.profile_end()
            assert rc == 0 and int(info[A.AI["KERNEL"]]) == A.AK["64"], (rc, info[:6])
            reps = int(info[A.AI["EXACT_WGS"]])
            if it:
                best.append(prof["flash_attention"][0])
        out[name] = {"kernel_us_median": round(float(np.median(best)) * 1e3, 1), "exact_workgroups": reps, "workgroups": 2 * 5 * 32}
    assert out["none_repeat"]["exact_workgroups"] == 0 and out["all_repeat"]["exact_workgroups"] == 320, out
    out["all_over_none"] = round(out["all_repeat"]["kernel_us_median"] / out["none_repeat"]["kernel_us_median"], 3)
    print(json.dumps({"lib": tsd._lib.LIB_PATH, **out}))


def measure(what, root, variant=None, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)]
    if variant:
        cmd += ["--variant", variant]
    env = {k: val for k, val in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library, unless one is named
    if lib:
        env["TSD_LIB"] = lib
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {what} {root} {variant} {lib} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {what} {root} {variant} {lib} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    got = os.path.realpath(rec.pop("lib"))
    assert got == os.path.realpath(lib) if lib else got.startswith(os.path.realpath(root) + os.sep), "the worker measured another library"
    return rec


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    nocheck = a.nocheck_lib if os.path.exists(a.nocheck_lib) else None
    arms = [("parent_1", "step", a.parent_root, "diffusion_sd15_torch", None), ("parent_2", "step", a.parent_root, "diffusion_sd15_torch", None),
            ("kind6", "step", ROOT, "diffusion_sd15_torch", None), ("sd2", "step", ROOT, "diffusion_sd2", None),
            ("attn", "attn", ROOT, None, None), ("peaked", "peaked", ROOT, None, None)]
    if nocheck:
        arms.append(("peaked_nocheck", "peaked", ROOT, None, nocheck))
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, what, root, variant, lib in arms[k:] + arms[:k]:
            rec[name] = measure(what, root, variant, lib)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {rec[k]['median']:.4f}" for k in ("parent_1", "parent_2", "kind6", "sd2")), flush=True)
    med = {n: [rd[n]["median"] for rd in rounds] for n in ("parent_1", "parent_2", "kind6", "sd2")}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    rb = [v / parent_median for v in med["kind6"]]
    inside = bool(lo <= float(np.median(rb)) <= hi)
    calls = {c: {"us_per_round": [rd["attn"]["calls"][c]["us"] for rd in rounds],
                 "us_median": round(float(np.median([rd["attn"]["calls"][c]["us"] for rd in rounds])), 2),
                 "tflops_median": round(float(np.median([rd["attn"]["calls"][c]["tflops"] for rd in rounds])), 1)} for c in rounds[0]["attn"]["calls"]}

    def peaked(name):
        return {k: {"per_round": [rd[name][k]["kernel_us_median"] for rd in rounds],
                    "us_median": round(float(np.median([rd[name][k]["kernel_us_median"] for rd in rounds])), 1)} for k in ("none_repeat", "all_repeat")} | \
            {"all_over_none_per_round": [rd[name]["all_over_none"] for rd in rounds],
             "all_over_none_median": round(float(np.median([rd[name]["all_over_none"] for rd in rounds])), 3)}

    out = {
        "what": "ms per step(), full-size UNet kinds, B=4 L=64 CFG on, 50 seeded DDPM steps; attention core calls at B=8 (tsd_debug_attn_bench); the "
                "(64, 5, 4096, 4096) launch at B=2 with no / every workgroup repeating; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "1_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "1_kind6_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in rb],
                                       "median": round(float(np.median(rb)), 5), "range": spread(rb), "inside_floor": inside},
        "2_sd2_step": {"sd2_ms_median": round(float(np.median(med["sd2"])), 4), "kind6_ms_median": round(float(np.median(med["kind6"])), 4),
                       "sd2_over_kind6_per_round": [round(x / y, 5) for x, y in zip(med["sd2"], med["kind6"])],
                       "sd2_class_ms_per_step_and_launches": rounds[-1]["sd2"]["class_ms_per_step_and_launches"],
                       "kind6_class_ms_per_step_and_launches": rounds[-1]["kind6"]["class_ms_per_step_and_launches"]},
        "3_attn_calls_b8": calls,
        "4_early_look": {"with": peaked("peaked"), "without": peaked("peaked_nocheck") if nocheck else None},
        "ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("1_parent_over_parent", "1_kind6_over_parent_median", "2_sd2_step", "3_attn_calls_b8", "4_early_look")}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    {"step": worker_step, "attn": worker_attn, "peaked": worker_peaked, None: driver}[a.worker]()
