"""Token merging on the device against tome_ref: the match inside a derived fp32 bound of the float64 cosine matrix, the tables equal to the
integer plan of the device's own node_max bits, merge / unmerge, the same bits run to run, per batch position and under the jitter build
(`python tests/test_gpu_tome.py jitter-child REPEATS` is its child), and kind 6 against the numpy forward merged by the recorded tables."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "stable-diffusion.mojo_amd"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import pytest

import tome_ref as T

pytestmark = pytest.mark.gpu
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
JITTER_REPEATS = 3
#        B, H, W, C, ratio, seed
CASES = [(1, 8, 8, 320, 0.5, 0),        # Nd = 16: a partial destination tile
         (2, 8, 24, 320, 0.75, 7),      # a rectangular grid
         (3, 16, 16, 640, 0.5, 0),      # two K chunks
         (1, 16, 16, 1280, 0.75, 7),    # the longest K loop
         (2, 32, 32, 320, 0.5, 7),      # several destination tiles and source workgroups
         (1, 64, 64, 320, 0.75, 0),     # Ns = 3072: more keys than threads in the select
         (1, 8, 8, 320, 0.13, 7)]       # rounds down to r = 8
IDS = [f"B{c[0]}-{c[1]}x{c[2]}-C{c[3]}-r{c[4]}-s{c[5]}" for c in CASES]
KEYS = ("node_max", "node_idx", "row_of", "start", "members")


def draw(B, H, W, C, seed):     # fp16 rows with a shared direction per 4 x 4 neighbourhood: scores spread over (0.3, 0.9), not around 0
    g = np.random.default_rng(seed)
    base = np.kron(g.standard_normal((B, -(-H // 4), -(-W // 4), C)), np.ones((1, 4, 4, 1)))[:, :H, :W]
    return (base + 0.7 * g.standard_normal((B, H, W, C))).reshape(B, H * W, C).astype(np.float16)


@functools.lru_cache(maxsize=None)
def planned(i):     # (x, the device's plan) of case i - computed once, shared, never modified
    import tsd
    B, H, W, C, ratio, seed = CASES[i]
    x = draw(B, H, W, C, 100 + i)
    return x, tsd.token_merge_plan(x, H, W, ratio, seed)


def check_plan(x, p, H, W, r, seed):     # both statements of the match for every row, the tables element for element; -> worst error / bound
    dst, src = T.partition(H, W, seed)
    e, worst = T.score_bound(x.shape[2]), 0.0
    for b in range(x.shape[0]):
        S, idx = T.cosine(x[b], dst, src), p["node_idx"][b]
        assert idx.min() >= 0 and idx.max() < len(dst)
        at = S[np.arange(len(src)), idx]
        err = np.abs(p["node_max"][b].astype(np.float64) - at)
        worst = max(worst, err.max() / e)
        assert (err <= e).all(), f"sample {b}: node_max is {err.max():.3e} from the float64 score, bound {e:.3e}"
        assert (at >= S.max(1) - 2 * e).all(), f"sample {b}: a partner {(S.max(1) - at).max():.3e} below the best, bound {2 * e:.3e}"
        want = T.plan(p["node_max"][b], idx, H, W, r, seed)
        assert all(np.array_equal(p[k][b], w) for k, w in zip(KEYS[2:], want)), b
    return worst


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_match_is_inside_the_fp32_bound_and_the_tables_are_the_integer_plan(gpu_ctx, i):
    (B, H, W, C, ratio, seed), (x, p) = CASES[i], planned(i)
    r = T.merged_count(ratio, H * W)
    assert p["rows"] == H * W - r and (i != len(CASES) - 1 or r == 8)
    worst = check_plan(x, p, H, W, r, seed)
    print(f"[tome] {IDS[i]}: worst match error / bound {worst:.3f}, / the sqrt(C) estimate {worst * T.score_bound(C) / T.score_typical(C):.3f}")


def test_equal_scores_take_the_smaller_index_a_zero_row_scores_zero_and_bad_arguments_are_refused(gpu_ctx, tsd_mod):
    H, W, ratio, seed = 16, 16, 0.25, 7
    dst, src = T.partition(H, W, seed)
    x = draw(1, H, W, 320, 31)
    x[0, dst[5]] = x[0, dst[40]] = x[0, dst[63]]        # three equal destinations: the winner among them is 5
    x[0, src[9]] = 0                                        # a zero source row
    x[0, src[100:172]] = x[0, dst[63]]                      # 72 equal sources at score 1: r = 64 cuts through them
    p = tsd_mod.token_merge_plan(x, H, W, ratio, seed)
    check_plan(x, p, H, W, 64, seed)
    idx, mx = p["node_idx"][0], p["node_max"][0]
    assert not np.isin(idx, (40, 63)).any() and (idx[100:172] == 5).all() and len(set(mx[100:172].tolist())) == 1
    assert idx[9] == 0 and mx[9] == 0 and (mx >= mx[100]).sum() > 64            # the threshold value has more holders than places
    assert (p["row_of"][0][src[100:164]] == (len(src) - 64) + 5).all() and (p["row_of"][0][src[164:172]] < len(src) - 64).all()
    bad = p["members"].copy(); bad[0, 3] = H * W            # a member outside the sample: refused before a kernel indexes with it
    for call, code in ((lambda: tsd_mod.token_merge_plan(x, H, W, 0.8), "TSD_E_ARG"), (lambda: tsd_mod.token_merge_plan(x, H, W, float("nan")), "TSD_E_ARG"),
                       (lambda: tsd_mod.token_merge_plan(draw(1, 6, 6, 320, 1), 6, 6, 0.5), "TSD_E_SHAPE"),
                       (lambda: tsd_mod.token_merge_rows(x, p["start"], bad), "TSD_E_ARG"),
                       (lambda: tsd_mod.token_unmerge_rows(x[:, :p["rows"]], np.full((1, H * W), p["rows"], np.int32)), "TSD_E_ARG")):
        with pytest.raises(tsd_mod.TsdError) as e:
            call()
        assert e.value.code == getattr(tsd_mod._lib, code)


def bitwise_cases(tsd, repeats):     # [(name, [digest per repeat])]: plan, merged rows and unmerged rows of three shapes
    out = []
    for i in (1, 2, 4):
        B, H, W, C, ratio, seed = CASES[i]
        x, v = draw(B, H, W, C, 100 + i), draw(B, H, W, C, 200 + i)
        ds = []
        for _ in range(repeats):
            p = tsd.token_merge_plan(x, H, W, ratio, seed)
            y = tsd.token_merge_rows(v, p["start"], p["members"])
            ds.append(hashlib.sha256(b"".join(a.tobytes() for a in [p[k] for k in KEYS] + [y, tsd.token_unmerge_rows(y, p["row_of"])])).hexdigest())
        out.append((IDS[i], ds))
    return out


@pytest.mark.parametrize("i", [1, 2, 5], ids=[IDS[1], IDS[2], IDS[5]])
def test_merge_is_inside_the_float64_bound_and_unmerge_is_the_gather(gpu_ctx, tsd_mod, i):
    (B, H, W, C, ratio, seed), (x, p) = CASES[i], planned(i)
    v = draw(B, H, W, C, 200 + i)
    y = tsd_mod.token_merge_rows(v, p["start"], p["members"])
    out, worst = tsd_mod.token_unmerge_rows(y, p["row_of"]), 0.0
    for b in range(B):
        ref, cnt, bound = T.merge(v[b], p["start"][b], p["members"][b])
        err, one, worst = np.abs(y[b].astype(np.float64) - ref), cnt == 1, max(worst, (np.abs(y[b].astype(np.float64) - ref) / bound).max())
        assert (err <= bound).all(), f"sample {b}: merged rows {(err / bound).max():.3f} of the bound"
        assert one.any() and (~one).any() and np.array_equal(y[b][one].view(np.uint16), v[b][p["members"][b][p["start"][b][:-1][one]]].view(np.uint16))
        assert np.array_equal(out[b].view(np.uint16), y[b][p["row_of"][b]].view(np.uint16))
        alone = tsd_mod.token_merge_plan(x[b:b + 1], H, W, ratio, seed)       # a sample alone gives the bits it gives at position b
        assert all(np.array_equal(alone[k][0], p[k][b]) for k in KEYS)
        assert np.array_equal(tsd_mod.token_merge_rows(v[b:b + 1], alone["start"], alone["members"])[0].view(np.uint16), y[b].view(np.uint16))
    print(f"[tome] {IDS[i]}: worst merge error / bound {worst:.3f}")


@pytest.mark.parametrize("i", [0, 1, 5], ids=[IDS[0], IDS[1], IDS[5]])
def test_nan_guard_bands_around_every_output_stay_untouched(gpu_ctx, tsd_mod, i):
    (B, H, W, C, ratio, seed), (x, p), G = CASES[i], planned(i), 64
    v, N = draw(B, H, W, C, 200 + i), H * W
    want = [p[k] for k in KEYS] + [tsd_mod.token_merge_rows(v, p["start"], p["members"])]
    want.append(tsd_mod.token_unmerge_rows(want[-1], p["row_of"]))
    bufs = [np.full(w.size + 2 * G, np.nan if w.dtype.kind == "f" else 0x7FC07FC0, w.dtype) for w in want]
    fill = [b.copy() for b in bufs]
    tsd_mod._lib.check(tsd_mod._lib.lib().tsd_debug_token_merge_run(gpu_ctx.h, x.ctypes.data, v.ctypes.data, B, H, W, C, ratio, seed, G,
                                                                    *(b.ctypes.data for b in bufs)))
    for name, b, f, w in zip(KEYS + ("y", "out"), bufs, fill, want):
        assert np.array_equal(b[G:-G].view(np.uint8), w.reshape(-1).view(np.uint8)), name
        assert np.array_equal(b[:G].view(np.uint8), f[:G].view(np.uint8)) and np.array_equal(b[-G:].view(np.uint8), f[-G:].view(np.uint8)), name


def test_same_bits_run_to_run_and_under_the_jitter_build(tsd_mod, gpu_ctx):
    here = bitwise_cases(tsd_mod, 3)
    for name, digests in here:
        assert len(set(digests)) == 1, f"{name}: {len(set(digests))} results in 3 runs"
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [t["name"] for t in there] == [n for n, _ in here]
    for (name, mine), theirs in zip(here, there):
        assert len(theirs["digests"]) == JITTER_REPEATS
        assert all(dg == mine[0] for dg in theirs["digests"]), f"{name}: the jitter build gave {len(set(theirs['digests']))} result(s), not the shipped bits"


KIND = "diffusion_sd15_torch"     # the model: kind 6 with a table


@pytest.fixture(scope="module")
def unet(gpu_ctx, tsd_mod):
    import freeu_ref as F
    from controlnet_ref import draw_params
    d = tsd_mod.Diffusion(params=draw_params(tsd_mod.param_specs(KIND), F.MODEL_SEED), variant=KIND)
    yield d
    d.model.close()


@pytest.mark.parametrize("shape, ratio", [((16, 16), (0.5, 0, 0, 0)), ((16, 32), (0.5, 0, 0, 0)), ((16, 16), (0.5, 0.5, 0, 0))],
                         ids=["16x16-l0", "16x32-l0", "16x16-l01"])
def test_forward_with_a_table_matches_the_numpy_forward_merged_by_the_recorded_tables(unet, tsd_mod, gpu_ctx, monkeypatch, shape, ratio):
    import freeu_ref as F
    from controlnet_ref import draw_params
    from oracle import ops
    from util import TOL_MODEL, rel_l2
    E, whole, seed = tsd_mod._lib.lib(), ops.self_attention, 11
    lat, ctx, temb = T.model_inputs(*shape)
    grid = {(shape[0] >> l) * (shape[1] >> l): (shape[0] >> l, shape[1] >> l) for l in range(2) if ratio[l]}     # tokens -> grid of a merging level
    plain = unet.forward(lat, ctx, temb)
    unet.set_token_merge((0, 0, 0, 0), seed)
    assert np.array_equal(unet.forward(lat, ctx, temb), plain)                    # a table of zeros: the parent's bits
    unet.set_token_merge(ratio, seed)
    try:
        assert unet.token_merge == (tuple(float(np.float32(v)) for v in ratio), seed)
        with pytest.raises(tsd_mod.TsdError):                                      # a level has a window or a ratio, not both
            unet.set_attn_window(8)
        assert E.tsd_debug_token_merge_record(gpu_ctx.h, 1) == 0
        out, tabs = unet.forward(lat, ctx, temb), []
        for k in range(E.tsd_debug_token_merge_record(gpu_ctx.h, 0)):
            rows = E.tsd_debug_token_merge_recorded(gpu_ctx.h, k, None, 0)
            t = np.empty((2, next(n for n in grid if rows == n - T.merged_count(0.5, n))), np.int32)
            assert E.tsd_debug_token_merge_recorded(gpu_ctx.h, k, t.ctypes.data, t.size) == rows
            tabs.append((rows, t))
        assert np.array_equal(unet.forward(lat, ctx, temb), out)
    finally:
        E.tsd_debug_token_merge_record(gpu_ctx.h, 0)
        unet.set_token_merge(None)
    assert np.array_equal(unet.forward(lat, ctx, temb), plain) and len(tabs) >= 2   # a NULL table: the parent's bits again
    for rows, t in tabs:                # structurally a plan: N - r rows, every destination owns its row, every token has one
        dst, _ = T.partition(*grid[t.shape[1]], seed)
        for b in range(2):
            assert t[b].min() == 0 and len(np.unique(t[b])) == rows == t[b].max() + 1 and np.array_equal(t[b][dst], rows - len(dst) + np.arange(len(dst)))
    P, state = draw_params(tsd_mod.param_specs(KIND), F.MODEL_SEED), {}

    def forward(miss):
        def merged(x, *a, **kw):         # mean by row -> the oracle's self attention -> gather, with the block's recorded table
            if x.shape[0] not in grid:
                return whole(x, *a, **kw)
            rows, t = tabs[state["k"]]
            state["k"] += 1
            row_of, s = t[state["b"]].astype(np.int64), np.zeros((rows, x.shape[1]))
            np.add.at(s, row_of, x)
            y = whole(s if miss == "sum" else s / np.bincount(row_of, minlength=rows)[:, None], *a, **kw)
            if miss == "own":            # merged sources copy the unmerged row of their own source index instead of their destination's
                keep, src = rows - x.shape[0] // 4, T.partition(*grid[x.shape[0]], seed)[1]
                m = row_of[src] >= keep
                row_of[src[m]] = np.arange(len(src))[m] % keep
            return y[row_of]

        monkeypatch.setattr(ops, "self_attention", merged)
        res = []
        for b in range(2):
            state.update(k=0, b=b)
            res.append(F.diffusion_freeu(P, lat[b], ctx[b], temb[b], None, tn=True))
        monkeypatch.setattr(ops, "self_attention", whole)
        return np.stack(res)

    d = dict({m: rel_l2(out, forward(m)) for m in (None, "sum", "own")}, plain=rel_l2(out, plain))
    print(f"[tome] {KIND} {shape} ratio {ratio}: rel_l2 to the merged numpy forward {d[None]:.3e}; to plain {d['plain']:.3e}, "
          f"to a sum instead of a mean {d['sum']:.3e}, to sources copied from their own index {d['own']:.3e} (tolerance {TOL_MODEL:.0e})")
    assert d[None] < TOL_MODEL < min(d["plain"], d["sum"], d["own"])


def _records(gpu_ctx, fn):
    gpu_ctx.profile_begin()
    try:
        fn()
        return [r[:5] for r in gpu_ctx.profile_records()]
    finally:
        gpu_ctx.profile_end()


def test_zero_and_null_tables_make_the_parents_launches_and_a_scribbled_workspace_changes_no_bit(gpu_ctx, tsd_mod, unet):
    args = T.model_inputs(16, 16)
    plain = _records(gpu_ctx, lambda: unet.forward(*args))
    try:
        unet.set_token_merge((0, 0, 0, 0), 9)
        assert _records(gpu_ctx, lambda: unet.forward(*args)) == plain
        unet.set_token_merge(None)
        assert _records(gpu_ctx, lambda: unet.forward(*args)) == plain
        unet.set_token_merge((0.5, 0.5, 0, 0), 9)
        outs = []
        for byte in (None, 0x00, 0xFF, 0x7B):      # the merged block reuses dead buffers of the plain block: nothing stale may be read
            if byte is not None:
                gpu_ctx.scribble(byte)
            outs.append(unet.forward(*args))
        assert np.isfinite(outs[0]).all() and all(np.array_equal(o, outs[0]) for o in outs[1:])
    finally:
        unet.set_token_merge(None)


def test_tiny_sd_with_a_table_keeps_its_fused_tails_and_drops_only_the_merged_heads(gpu_ctx, tsd_mod):
    d, B, L = tsd_mod.Diffusion(seed=5), 2, 16
    lat, ctx, temb = T.model_inputs(L, L, B, kind="diffusion_sd15_torch")
    try:
        plain = _records(gpu_ctx, lambda: d.forward(lat, ctx, temb))
        d.set_token_merge(0.5)
        with_t = _records(gpu_ctx, lambda: d.forward(lat, ctx, temb))
    finally:
        d.set_token_merge(None)
        d.model.close()
    chain = lambda recs, head: [r for r in recs if r[0] == "attn_tail_chain" and r[3] == head]      # K = 1: the head kernel, 0: the tail
    assert chain(with_t, 0) == chain(plain, 0) and len(chain(plain, 0)) > 0
    assert chain(with_t, 1) == [r for r in chain(plain, 1) if r[1] != B * L * L] and len(chain(with_t, 1)) < len(chain(plain, 1))
    assert len([r for r in with_t if r[0] == "elementwise"]) - len([r for r in plain if r[0] == "elementwise"]) == \
        3 * (len(chain(plain, 1)) - len(chain(with_t, 1)))       # plan, merge, unmerge per merged block; no other class of launch moves there


def test_cfg_session_equals_the_host_loop_and_a_switch_inside_an_open_session_matches_fresh_runs(gpu_ctx, tsd_mod, unet, monkeypatch):
    import test_gpu_controlnet as TC           # the host-driven loop and the session driver ...
    monkeypatch.setattr(TC, "S_STEPS", 4)      # ... on a schedule of four steps
    case, inputs, table = TC.S_CASES[0], TC._s_inputs(2400), (0.5, 3)          # seeded DDPM, CFG, four steps at 16 x 16 latents
    loop = lambda x0, first, n=1: TC.host_loop(tsd_mod, gpu_ctx, unet, None, case, True, inputs, lambda i: None, x0=x0, first=first, steps=first + n)
    s = TC._open(tsd_mod, unet, True, case[1], case[2], case[3])
    try:
        s.upload(inputs[0], inputs[1], inputs[2], None, cfg_scale=TC.S_CFG_SCALE)       # the workspace is sized with no table
        s.set_seeds(TC.S_SEEDS)
        s.step(0); g0 = s.latents()
        unet.set_token_merge(*table)
        s.step(1); g1 = s.latents()
        unet.set_token_merge(None)
        s.step(2); g2 = s.latents()
        s.close()
        p0, p2 = loop(None, 0)[0], loop(g1, 2)[0]
        unet.set_token_merge(*table)
        got, want, w1 = TC.session_run(tsd_mod, unet, None, case, True, inputs, None), loop(None, 0, TC.S_STEPS), loop(g0, 1)[0]
    finally:
        s.close()
        unet.set_token_merge(None)
    assert TC.S_STEPS == 4 and len(got) == 4 and all(TC._same(a, b) for a, b in zip(got, want))
    assert TC._same(g0, p0) and TC._same(g1, w1) and TC._same(g2, p2) and not TC._same(g1, loop(g0, 1)[0])


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    import tsd
    tsd.set_strict(True)
    for _name, _digests in bitwise_cases(tsd, int(sys.argv[2])):
        print(json.dumps({"name": _name, "digests": _digests}), flush=True)
