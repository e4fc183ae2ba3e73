"""ms per denoise step of a device session with a given sampler at the headline size (B = 8, L = 64, 50 steps), CFG off and on.

  python scripts/bench_sampler_step.py --sampler ddpm|ddim|dpmpp_2m [--spacing leading|trailing] [--eta E] [--passes P] [--root DIR]

One JSON line: per CFG setting the ms/step of every timed pass (hipEvents on the library's stream around the 50 enqueued steps) and
their median.  --root names the tree whose package and library are measured (default: this one), so two checkouts can be run
alternately from one driver - same-box pairs; a tree without `Session.set_sampler` can only be asked for "ddpm"."""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--sampler", default="ddpm")
ap.add_argument("--spacing", default="leading")
ap.add_argument("--eta", type=float, default=0.0)
ap.add_argument("--passes", type=int, default=4)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.join(a.root, "stable-diffusion.mojo_amd"))
import tsd  # noqa: E402
from tsd import rng  # noqa: E402

SEED, B, L, T = 1234, 8, 64, 77
tsd.set_strict(True)
unet = tsd.Diffusion(seed=SEED)
dctx = tsd.default_context()
nl = B * 4 * L * L
lat = rng.normal(SEED, 2, nl).reshape(B, 4, L, L)
ctx = rng.normal(SEED, 5, B * T * 768).reshape(B, T, 768)
uctx = rng.normal(SEED, 6, B * T * 768).reshape(B, T, 768)
out = {"tag": a.tag, "sampler": a.sampler, "spacing": a.spacing, "eta": a.eta, "B": B, "L": L, "steps": a.steps, "lib": tsd._lib.LIB_PATH}
for cfg in (False, True):
    sess = tsd.Session(unet.model, None, B, L, T, cfg=cfg)
    if (a.sampler, a.spacing, a.eta) != ("ddpm", "leading", 0.0):
        sess.set_sampler(a.sampler, a.eta, a.spacing)
    sess.set_schedule(1000, a.steps, 0)
    n = sess.num_steps
    noise = rng.normal(SEED, 3, n * nl).reshape(n, B, 4, L, L)
    ms = []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        sess.upload(lat, ctx, uctx if cfg else None, noise, 7.5)
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    assert np.isfinite(sess.latents()).all()
    sess.close()
    out["cfg_on" if cfg else "cfg_off"] = {"ms_per_step": [round(v, 4) for v in ms], "median": round(float(np.median(ms)), 4)}
print(json.dumps(out))
