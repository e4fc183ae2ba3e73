"""What IP-Adapter Plus costs, and that a plain denoise step costs what it did: interleaved same-box rounds, one fresh process per
measurement (the pattern of scripts/bench_ip_adapter_step.py).

  python scripts/bench_ip_plus.py --parent-root DIR [--rounds R] [--passes P] [--resample-rounds R2] [--out FILE]

DIR is a checkout of the parent commit with its library built.  Full-size UNet, B = 4, L = 64, CFG on, 50 seeded DDPM steps; every round
runs five fresh processes one after the other, in an order that rotates from round to round: the parent tree's step() twice, then this
tree's step() without an adapter, with a kind-20 adapter (N = 4 tokens) and with a plus adapter (N = 16 tokens), scale 1 on both CFG
halves.  Each process times P passes of the 50 enqueued steps with hipEvents on the library's stream (after one warm-up pass) and reports
their median.  Every process has its own time limit and the first failure ends the run.  Recorded:
  (a) the parent against the parent (the A/A spread of this box) and this tree's plain step() against the parent's median - ACCEPTANCE:
      the median ratio lies inside the A/A spread of the same run (nothing existing got slower); at least eight rounds;
  (b) the adapted step() with the plus adapter beside the kind-20 one and beside the plain step: ratios and us per step, reported, not
      gated (k_ip_attn_add computes one 16-key tile whatever N is, so N = 16 is expected to cost what N = 4 does);
  (c) tsd_ip_adapter_resample at S = 257, B = 1, 4, 16 (host in, host out, synchronous: the copies are included), beside
      tsd_clip_vision_forward with hidden_out at the same B on a 224 x 224 image, in ms per call: median and range over R2 rounds of a
      worker's median of 20 calls after two warm-up calls; and the launches of one resample call from the profile records.
Writes FILE (default profiles/ip_plus_pairs.json); exits 1 when (a) is outside the floor.

  python scripts/bench_ip_plus.py --worker --root DIR [--adapter plain|plus]        one step measurement, one JSON line
  python scripts/bench_ip_plus.py --call-worker --which resample|vision --B B        one (c) measurement, one JSON line"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--worker", action="store_true")
ap.add_argument("--call-worker", action="store_true")
ap.add_argument("--which", default="resample")
ap.add_argument("--B", type=int, default=1)
ap.add_argument("--root", default=ROOT)
ap.add_argument("--adapter", default=None, help="worker: set_ip_adapter with an adapter of this kind at scale 1 (absent: no adapter)")
ap.add_argument("--parent-root")
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--resample-rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--worker-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_plus_pairs.json"))
a = ap.parse_args()
SEED, B, L, T, S_HIDDEN = 1234, 4, 64, 77, 257


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
    ip = tok = utok = None
    if a.adapter == "plain":  # the parent's library is never asked for what it does not have
        ip = tsd.IPAdapter(seed=SEED)
        emb = rng.normal(SEED, 7, B * 1024).reshape(B, 1024)
        tok, utok = ip.project(emb), ip.project(np.zeros_like(emb))
    elif a.adapter == "plus":
        ip = tsd.IPAdapter(seed=SEED, variant="ip_adapter_plus_sd15")
        tok = ip.resample(rng.normal(SEED, 7, B * S_HIDDEN * 1280).reshape(B, S_HIDDEN, 1280))
        utok = ip.resample(rng.normal(SEED, 8, B * S_HIDDEN * 1280).reshape(B, S_HIDDEN, 1280))
    ms = []
    for p in range(a.passes + 1):  # pass 0 warms every shape up
        sess.upload(lat, ctx, uctx, None, 7.5)
        sess.set_seeds([100 + b for b in range(B)])
        sess.add_noise_seeded(0)
        if ip is not None and p == 0:
            sess.set_ip_adapter(ip, tok, utok, scale=1.0)   # it outlives the later uploads
        dctx.synchronize()
        dctx.timer_start()
        for i in range(n):
            sess.step(i)
        t = dctx.timer_stop()
        if p:
            ms.append(t / n)
    assert np.isfinite(sess.latents()).all()
    sess.close()
    print(json.dumps({"lib": tsd._lib.LIB_PATH, "adapter": a.adapter, "n_tokens": None if tok is None else int(tok.shape[1]),
                      "ms_per_step": [round(v, 4) for v in ms], "median": round(float(np.median(ms)), 4)}))


def call_worker():
    sys.path.insert(0, os.path.join(ROOT, "stable-diffusion.mojo_amd"))
    import tsd
    tsd.set_strict(True)
    g = np.random.default_rng(a.B)
    launches = None
    if a.which == "resample":
        ip = tsd.IPAdapter(seed=SEED, variant="ip_adapter_plus_sd15")
        x = g.standard_normal((a.B, S_HIDDEN, 1280)).astype(np.float32)
        call = lambda: ip.resample(x)  # noqa: E731
    else:
        enc = tsd.CLIPVision(seed=SEED)
        x = g.uniform(0.0, 255.0, size=(a.B, 3, 224, 224)).astype(np.float32)
        call = lambda: enc.forward(x, hidden=True)[1]  # noqa: E731
    for _ in range(2):
        out = call()
    assert np.isfinite(out).all()
    ms = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    dctx = tsd.default_context()
    dctx.profile_begin()
    try:
        call()
        recs = dctx.profile_records()
    finally:
        dctx.profile_end()
    by_class = {}
    for r in recs:
        by_class[str(r[0])] = by_class.get(str(r[0]), 0) + 1
    launches = {"records": len(recs), "by_class": by_class}
    print(json.dumps({"which": a.which, "B": a.B, "ms": statistics.median(ms), "ms_min": min(ms), "launches": launches}), flush=True)


def _run(cmd, what, root=None):
    env = {k: val for k, val in os.environ.items() if k != "TSD_LIB"}  # each tree measures its own library
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=a.worker_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"worker {what} ran past its {a.worker_timeout} s limit: nothing more is started")
    if r.returncode != 0:  # nothing more is started on the GPU after a failed measurement
        sys.exit(f"worker {what} exited {r.returncode}:\n{r.stderr[-2000:]}")
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    if root is not None:
        assert os.path.realpath(rec.pop("lib")).startswith(os.path.realpath(root) + os.sep), "the worker measured another tree's library"
    return rec


def measure(root, adapter):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--passes", str(a.passes), "--steps", str(a.steps)] + \
        (["--adapter", adapter] if adapter is not None else [])
    return _run(cmd, f"{root} adapter={adapter}", root)


def measure_call(which, nb):
    return _run([sys.executable, os.path.abspath(__file__), "--call-worker", "--which", which, "--B", str(nb), "--iters", str(a.iters)], f"{which} B={nb}")


def spread(v):
    return [round(float(min(v)), 5), round(float(max(v)), 5)]


def driver():
    if not a.parent_root:
        ap.error("--parent-root DIR (a checkout of the parent commit with its library built) is required")
    arms = [("parent_1", a.parent_root, None), ("parent_2", a.parent_root, None), ("step_plain", ROOT, None), ("step_kind20", ROOT, "plain"),
            ("step_plus", ROOT, "plus")]
    rounds = []
    t0 = time.time()
    for r in range(a.rounds):
        rec = {}
        k = r % len(arms)
        for name, root, adapter in arms[k:] + arms[:k]:
            rec[name] = measure(root, adapter)
        rounds.append(rec)
        print(f"round {r}: " + "  ".join(f"{k} {v['median']:.4f}" for k, v in sorted(rec.items())), flush=True)
    med = {arm[0]: [rd[arm[0]]["median"] for rd in rounds] for arm in arms}
    aa = [p2 / p1 for p1, p2 in zip(med["parent_1"], med["parent_2"])]
    aa_sym = aa + [1.0 / v for v in aa]
    lo, hi = min(aa_sym), max(aa_sym)
    parent_median = float(np.median(med["parent_1"] + med["parent_2"]))
    ra = [v / parent_median for v in med["step_plain"]]
    inside = bool(lo <= float(np.median(ra)) <= hi)

    def pair(x, y):
        rt = [p / q for p, q in zip(med[x], med[y])]
        dl = [1e3 * (p - q) for p, q in zip(med[x], med[y])]
        return {"per_round": [round(v, 5) for v in rt], "median": round(float(np.median(rt)), 5), "range": spread(rt),
                "us_per_step_added_median": round(float(np.median(dl)), 1), "us_per_step_added_range": spread(dl)}
    calls = {}
    cases = [(w, nb) for nb in (1, 4, 16) for w in ("resample", "vision")]
    for r in range(a.resample_rounds):
        k = r % len(cases)
        for w, nb in cases[k:] + cases[:k]:
            rec = measure_call(w, nb)
            c = calls.setdefault(f"{w}_B{nb}", {"ms_rounds": [], "launches": rec["launches"]})
            c["ms_rounds"].append(round(rec["ms"], 4))
            print(f"round {r} {w} B={nb}: {rec['ms']:.3f} ms, {rec['launches']['records']} launch records", flush=True)
    for c in calls.values():
        c["ms_median"], c["ms_range"] = round(statistics.median(c["ms_rounds"]), 4), spread(c["ms_rounds"])
    out = {
        "what": "(a), (b): ms per step(), full-size UNet, B=4 L=64 CFG on, 50 seeded DDPM steps; adapter arms: set_ip_adapter(scale 1) with a kind-20 "
                "adapter (N = 4) and a plus adapter (N = 16); (c): ms per synchronous host-in / host-out call at S = 257 / 224x224; interleaved "
                "same-box rounds, one fresh process per measurement",
        "rounds": len(rounds), "passes": a.passes, "resample_rounds": a.resample_rounds, "iters": a.iters,
        "a_parent_over_parent": {"per_round": [round(v, 5) for v in aa], "spread": [round(lo, 5), round(hi, 5)]},
        "a_step_plain_over_parent_median": {"parent_median_ms": round(parent_median, 4), "per_round": [round(v, 5) for v in ra],
                                            "median": round(float(np.median(ra)), 5), "range": spread(ra), "inside_floor": inside},
        "b_step_plus_over_kind20": pair("step_plus", "step_kind20"),
        "b_step_plus_over_plain": pair("step_plus", "step_plain"),
        "b_step_kind20_over_plain": pair("step_kind20", "step_plain"),
        "c_calls": calls,
        "ms_per_step": {k: {"per_round_median": v, "median": round(float(np.median(v)), 4)} for k, v in med.items()},
        "per_round": rounds, "seconds": round(time.time() - t0, 1), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("a_parent_over_parent", "a_step_plain_over_parent_median", "b_step_plus_over_kind20", "b_step_plus_over_plain",
                                          "b_step_kind20_over_plain")}))
    print(json.dumps({k: {"ms_median": v["ms_median"], "ms_range": v["ms_range"], "launches": v["launches"]["records"]} for k, v in calls.items()}))
    sys.exit(0 if inside else 1)


if __name__ == "__main__":
    if a.worker:
        worker()
    elif a.call_worker:
        call_worker()
    else:
        driver()
