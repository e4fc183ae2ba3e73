"""What masked denoising costs a denoise step, and that a session without it costs what it did: interleaved same-box pairs at the
headline size (B = 8, L = 64, 50 DDPM steps, CFG off).

  python scripts/bench_inpaint_step.py --parent-root DIR [--rounds R] [--passes P] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Every round runs four fresh processes one after the other, in an order
that rotates from round to round: the parent tree twice, this tree without inpainting, this tree with it.  Each process times P passes
of the 50 enqueued steps with hipEvents on the library's stream (after one warm-up pass) and reports their median.  Recorded:
  (a) parent against parent, the A/A spread of this box;
  (b) this tree unmasked against the parent - must lie inside the spread of (a): the unmasked step gains a host branch only;
  (c) this tree masked against this tree unmasked - the cost of the blend launch;
  (d) the ms/step themselves.
Writes FILE (default profiles/inpaint_step_pairs.json) and exits 1 when (b) is outside (a).

  python scripts/bench_inpaint_step.py --worker --root DIR [--masked]     one measurement, one JSON line (what the driver starts)"""
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
ap.add_argument("--masked", action="store_true")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--passes", type=int, default=4)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_step_pairs.json"))
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
    noise = rng.normal(SEED, 3, n * nl).reshape(n, B, 4, L, L)
    if a.masked:  # the left half is regenerated, the right half kept, a soft column between them
        mask = np.zeros((B, L, L), dtype=np.float32)
        mask[:, :, : L // 2] = 1.0
        mask[:, :, L // 2] = 0.5
        known = rng.normal(SEED, 7, nl).reshape(B, 4, L, L)
        z = rng.normal(SEED, 8, nl).reshape(B, 4, L, L)
    ms = []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        sess.upload(lat, ctx, None, noise, 7.5)
        if a.masked:
            sess.set_inpaint(mask, known, z)
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    out = sess.latents()
    assert np.isfinite(out).all()
    if a.masked:
        assert np.array_equal(out[:, :, :, L // 2 + 1:], known[:, :, :, L // 2 + 1:])  # the kept region is the known latents
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "masked": a.masked, "ms_per_step": [round(v, 4) for v in ms],
                      "median": round(float(np.median(ms)), 4)}))


def measure(root, masked):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)]
    env = {k: v for k, v in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    r = subprocess.run(cmd + (["--masked"] if masked else []), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=300)
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {root} masked={masked} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, False), ("parent_2", a.parent_root, False), ("new_unmasked", ROOT, False), ("new_masked", ROOT, True)]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        for name, root, masked in arms[r % 4:] + arms[: r % 4]:
            rec[name] = measure(root, masked)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {k: [rd[k]["median"] for rd in rounds] for k, _, _ in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    b = [n / p for n, p in zip(med["new_unmasked"], med["parent_1"])]
    c = [m / u for m, u in zip(med["new_masked"], med["new_unmasked"])]
    b_med = float(np.median(b))
    out = {
        "what": "ms per denoise step, B=8 L=64 50 DDPM steps CFG off; interleaved same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes,
        "a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(min(aa_sym), 5), round(max(aa_sym), 5)]},
        "b_new_unmasked_over_parent": {"per_round": [round(v, 5) for v in b], "median": round(b_med, 5),
                                       "inside_a": bool(min(aa_sym) <= b_med <= max(aa_sym))},
        "c_new_masked_over_new_unmasked": {"per_round": [round(v, 5) for v in c], "median": round(float(np.median(c)), 5),
                                           "ms_per_step_added_median": round(float(np.median(
                                               [m - u for m, u in zip(med["new_masked"], med["new_unmasked"])])), 4)},
        "d_ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_parent_over_parent", "b_new_unmasked_over_parent", "c_new_masked_over_new_unmasked")}))
    sys.exit(0 if out["b_new_unmasked_over_parent"]["inside_a"] else 1)


if __name__ == "__main__":
    worker() if a.worker else driver()
