"""GPU: the GEMM / conv3x3 kernel (csrc/kernels_gemm.hip) held to an fp64 reference element-wise (tests/gemm_ref.py) through
tsd_debug_gemm_run - every launch the product makes (recorded, then replayed on seeded operands with the dispatcher's choice),
every tile configuration on the shapes where tiles break, the dispatcher-only modes and the documented refusals.  Outputs sit
between NaN guard bands and are pre-filled with NaN: a stray store or an element no tile wrote fails."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import gemm_ref as G
import replay

pytestmark = pytest.mark.gpu
E = G.EPI
SEED = 1234
_i64p = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def ctx(gpu_ctx, tsd_mod):
    c = tsd_mod.Context(gpu_ctx.device)
    yield c
    c.close()


def run(ctx, d, ops, cfg=-1):
    """(status, outputs {C, VT, GN}, info [cfg, ways, guard / gap writes])."""
    return replay.run("tsd_debug_gemm_run", ctx, d, ops, G.GO, G.INPUTS, G.OUTPUTS, G.dtype_of, G.extents, extra=(cfg,))


def planned(ctx, d, cfg=-1):
    """(configuration, split-K slices) of the host plan for d on this context: tsd_debug_gemm_plan, no launch."""
    d = np.ascontiguousarray(d, np.int64)
    p = np.zeros(G.GP["COUNT"], np.int64)
    rc = replay.lib().tsd_debug_gemm_plan(ctx.h, d.ctypes.data_as(_i64p), len(d), cfg, p.ctypes.data_as(_i64p))
    assert rc == 0, f"cfg {cfg}: plan status {rc}: {replay.lib().tsd_last_error().decode()}"
    return int(p[G.GP["CFG"]]), int(p[G.GP["WAYS"]])


def verify(ctx, d, cfg=-1, seed=0, rows=None, twice=False):
    """Run d on seeded operands and hold it to the reference; returns info."""
    ops = G.make_operands(d, seed)
    rc, outs, info = run(ctx, d, ops, cfg)
    assert rc == 0, f"cfg {cfg}: status {rc}: {replay.lib().tsd_last_error().decode()}"
    assert info[2] == 0, f"cfg {info[0]}: {info[2]} guard / pitch-gap elements written"
    M, B = int(d[G.GD["M"]]), int(d[G.GD["BATCH"]])
    rows = np.arange(M * B) if rows is None else rows
    fails = G.check(d, ops, outs, rows)
    if int(d[G.GD["EPI"]]) & E["GNSTATS"]:
        fails += G.check_gn(d, outs["C"], outs["GN"])
    assert not fails, f"cfg {info[0]} ways {info[1]}: " + "; ".join(fails)
    if twice:
        rc2, outs2, info2 = run(ctx, d, ops, cfg)
        assert rc2 == 0 and (info2[:2] == info[:2]).all()
        for s in outs:
            assert np.array_equal(outs[s].view(np.uint8), outs2[s].view(np.uint8)), f"second replay of {s} differs"
    return info


# ---- (a) production replay ---------------------------------------------------------------------------------------------------
def _recorded(ctx, fn):
    lib = replay.lib()
    lib.tsd_debug_gemm_record(ctx.h, 1)
    try:
        fn()
    finally:
        n = lib.tsd_debug_gemm_record(ctx.h, 0)
    out = []
    for i in range(n):
        d = np.zeros(G.COUNT, np.int64)
        assert lib.tsd_debug_gemm_recorded(ctx.h, i, d.ctypes.data_as(_i64p), G.COUNT) == G.COUNT
        out.append(d)
    return out


@pytest.fixture(scope="module")
def production(ctx, tsd_mod):
    rng = np.random.default_rng(SEED)
    descs = []

    def step(unet, B, L, cfg):
        lat = rng.standard_normal((B, 4, L, L)).astype(np.float32)
        cond = rng.standard_normal((B, 77, 768)).astype(np.float32)
        s = tsd_mod.Session(unet.model, None, B, L, 77, cfg=cfg)
        try:
            s.set_schedule(1000, 2, 0)
            s.upload(lat, cond, cond[::-1].copy() if cfg else None, None, cfg_scale=7.5)
            s.step(0)
            s.latents()
        finally:
            s.close()

    unet = tsd_mod.Diffusion(seed=SEED, ctx=ctx)
    descs += _recorded(ctx, lambda: step(unet, 8, 64, False))     # BASELINE configs[1]
    descs += _recorded(ctx, lambda: step(unet, 8, 64, True))      # CFG: the UNet at batch 16
    del unet
    dec = tsd_mod.Decoder(seed=SEED, ctx=ctx)
    descs += _recorded(ctx, lambda: dec.forward(rng.standard_normal((1, 4, 64, 64)).astype(np.float32)))
    del dec
    enc = tsd_mod.Encoder(seed=SEED, ctx=ctx)
    img = rng.uniform(-1, 1, (1, 3, 512, 512)).astype(np.float32)
    descs += _recorded(ctx, lambda: enc.forward(img, rng.standard_normal((1, 4, 64, 64)).astype(np.float32)))
    del enc
    full = tsd_mod.Diffusion(seed=SEED, ctx=ctx, variant="diffusion_sd15")
    descs += _recorded(ctx, lambda: step(full, 4, 64, False))    # asks for 4 slices at K >= 8192
    del full
    uniq = {}
    for d in descs:
        uniq.setdefault(tuple(int(x) for x in d), d)
    return list(uniq.values())


def test_production_launches_replay_within_the_fp64_bound(ctx, production):
    cov = Counter()
    assert len(production) > 20
    for i, d in enumerate(production):
        info = verify(ctx, d, -1, seed=100 + i, rows=G.sample_rows(d, 7 + i), twice=True)
        assert (int(info[0]), int(info[1])) == (int(d[G.GD["CFG"]]), int(d[G.GD["WAYS"]])), "replay chose another tile / split"
        assert planned(ctx, d) == (int(info[0]), int(info[1])), "the plan is not what ran"
        cov[(int(info[0]), int(info[1]))] += 1
    assert replay.lib().tsd_debug_splitk_errors(ctx.h) == 0
    print("\nreplayed launches per (configuration, split-K ways):")
    for (cfg, ways), n in sorted(cov.items()):
        print(f"  cfg {cfg:3d}  ways {ways}  : {n}")
    cfgs = {c for c, _ in cov}
    assert {51, 53, 54, 47, 5} <= cfgs, cfgs
    assert len({w for _, w in cov if w > 1}) >= 2, cov


# ---- (b) configuration sweep ----------------------------------------------------------------------------------------------------
N160, N128, THIN = G.N160, G.N128, G.THIN
BNW, SPLITS, _sweep_cases, _vt_desc = G.BNW, G.SPLITS, G._sweep_cases, G._vt_desc


SWEEP = _sweep_cases()


def test_every_tile_configuration_matches_the_fp64_reference(ctx):
    counts = Counter()
    for name, d, cfgs in SWEEP:
        epi = int(d[G.GD["EPI"]])
        gn_ran = set()
        for cfg in cfgs:
            if cfg == 30 and int(d[G.GD["N"]]) % 160:
                continue
            if epi & E["GNSTATS"]:
                rc, outs, info = run(ctx, d, G.make_operands(d, 1), cfg)
                if rc != 0:  # the forced tile cannot emit these statistics: refused, nothing written
                    assert info[2] == 0 and all(np.isnan(o.astype(np.float32)).all() for o in outs.values()), f"{name} cfg {cfg}"
                    continue
                gn_ran.add(cfg)
            try:
                info = verify(ctx, d, cfg, seed=cfg)
                assert planned(ctx, d, cfg) == (int(info[0]), int(info[1])), "the plan is not what ran"
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from None
            counts[cfg] += 1
        if epi & E["GNSTATS"]:  # exactly the tiles whose wave columns hold whole groups take the statistics
            cpg = int(d[G.GD["N"]]) // int(d[G.GD["GN_GROUPS"]])
            want = {c for c in cfgs if BNW[c] % cpg == 0}
            assert want and gn_ran == want, f"{name}: statistics ran on {sorted(gn_ran)}, expected {sorted(want)}"
    assert replay.lib().tsd_debug_splitk_errors(ctx.h) == 0
    print("\nsweep cases per configuration: " + ", ".join(f"{c}: {n}" for c, n in sorted(counts.items())))
    assert set(counts) >= set(N160 + N128 + THIN + (30, 32)), counts


# ---- (c) dispatcher-only modes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,ways", SPLITS, ids=[s[0] for s in SPLITS])
def test_split_k_matches_the_fp64_reference(ctx, name, d, ways):
    info = verify(ctx, d, -1, seed=3, twice=True)
    assert int(info[1]) == ways, f"{name}: {int(info[1])} slices"
    assert replay.lib().tsd_debug_splitk_errors(ctx.h) == 0


def test_optin_256_row_split_matches_the_fp64_reference(gpu_ctx, tsd_mod, monkeypatch):
    monkeypatch.setenv("TSD_GEMM_SK256", "3")
    c = tsd_mod.Context(gpu_ctx.device)
    monkeypatch.delenv("TSD_GEMM_SK256")
    try:
        d = G.dense_desc(M=1024, N=1280, K=5120, epi=E["BIAS_N"] | E["RESIDUAL"], rps_hint=256)
        info = verify(c, d, -1, seed=4, twice=True)
        assert (int(info[0]), int(info[1])) == (51, 4)
        assert replay.lib().tsd_debug_splitk_errors(c.h) == 0
    finally:
        c.close()


def test_vt_tail_matches_the_fp64_reference(ctx):
    verify(ctx, _vt_desc(), -1, seed=5, twice=True)


# ---- (d) refusals -------------------------------------------------------------------------------------------------------------
def _refusals():
    gn = dict(gn_groups=32, gn_rps=256, gn_nslab=8)
    return [
        ("gn_with_geglu", G.dense_desc(M=512, N=640, K=128, epi=E["BIAS_N"] | E["GEGLU"] | E["GNSTATS"], **gn), -1),
        ("gn_with_f32", G.dense_desc(M=512, N=640, K=128, epi=E["BIAS_N"] | E["OUT_F32"] | E["GNSTATS"], **gn), -1),
        ("halo_on_stride2", G.conv_desc(B=1, Hs=8, Ws=128, Cin=64, N=256, stride=2, epi=E["BIAS_N"]), 32),
        ("vt_forced", _vt_desc(), 7),
        ("k0_not_multiple_of_64", G.dense_desc(M=64, N=160, K=192, K0=96, epi=E["BIAS_N"]), -1),
    ]


@pytest.mark.parametrize("name,d,cfg", _refusals(), ids=[r[0] for r in _refusals()])
def test_refused_launches_leave_the_outputs_untouched(ctx, name, d, cfg):
    rc, outs, info = run(ctx, d, G.make_operands(d, 6), cfg)
    assert rc != 0, f"{name} was not refused"
    assert info[2] == 0
    replay.assert_untouched(outs, name)


# ---- (4) the folded GEGLU-2 / conv_out weights against fp64 -------------------------------------------------------------------
def _fold(model, block):
    """(C, folded weight [C][5C] fp16, bias [C] fp32) of a prepared model's attention block; C = 0 when it does not fold."""
    lib = replay.lib()
    C_ = lib.tsd_debug_model_fold(model.h, block, None, None)
    assert C_ >= 0, lib.tsd_last_error().decode()
    if not C_:
        return 0, None, None
    wf = np.empty(C_ * 5 * C_, np.float16)
    bf = np.empty(C_, np.float32)
    assert lib.tsd_debug_model_fold(model.h, block, wf.ctypes.data, bf.ctypes.data_as(C.POINTER(C.c_float))) == C_
    return C_, wf.reshape(C_, 5 * C_), bf


def _fold_params(params, block):
    n = f"unet.layer{block + 1}"
    return (params[n + ".layer10.kernel"], params[n + ".layer10.bias"], params[n + ".layer9.weight"], params[n + ".layer9.bias"])


def _check_fold(wf, bf, wo32, bo, w232, b2):
    """wf = fp16(fp32 index-order sum of wo . w2): within one fp16 rounding of the fp64 product plus the C-term fp32 sum bound;
    the copied W_out columns bit-exact; the fp32 bias within its (C + 1)-add bound."""
    C_ = wo32.shape[0]
    wo = wo32.reshape(C_, C_).astype(np.float16).astype(np.float64)
    w2 = w232.astype(np.float16).astype(np.float64)
    assert np.array_equal(wf[:, 4 * C_:].view(np.uint16), wo.astype(np.float16).view(np.uint16)), "copied W_out columns differ"
    ref, mag = wo @ w2, np.abs(wo) @ np.abs(w2)
    bd = 2.0 ** -11 * np.abs(ref) + (1 + 2.0 ** -11) * C_ * G.U32 * mag + 2.0 ** -25
    err = np.abs(wf[:, :4 * C_].astype(np.float64) - ref)
    assert (err <= bd).all(), f"folded weight: {int((~(err <= bd)).sum())} elements off, worst {np.max(err / bd):.3g} x bound"
    rb = wo @ b2.astype(np.float64) + bo.astype(np.float64)
    bb = (C_ + 1) * G.U32 * (np.abs(wo) @ np.abs(b2.astype(np.float64)) + np.abs(bo))
    assert (np.abs(bf.astype(np.float64) - rb) <= bb).all(), "folded bias off"


def _param_index(model, name):
    return [s[0] for s in model.specs].index(name)


def test_folded_weights_match_fp64_and_heavy_tails_replay(ctx, tsd_mod, unet_params):
    unet = tsd_mod.Diffusion(seed=SEED, ctx=ctx)
    try:
        unet.model.prepare()
        blocks, b = [], 0
        while True:
            c_ = replay.lib().tsd_debug_model_fold(unet.model.h, b, None, None)
            if c_ < 0:
                break
            if c_ > 0:
                blocks.append((b, c_))
            b += 1
        sizes = {c for _, c in blocks}
        assert {640, 1280} <= sizes, blocks
        picked = [next(b for b, c in blocks if c == 640), next(b for b, c in blocks if c == 1280)]
        for blk in picked:
            C_, wf, bf = _fold(unet.model, blk)
            _check_fold(wf, bf, *_fold_params(unet_params, blk))
        # heavy tails: a few conv_out rows and geglu2 columns x 30, then the fold again and its GEMM replayed with those weights
        blk = picked[0]
        wo, bo, w2, b2 = (np.array(x, np.float32) for x in _fold_params(unet_params, blk))
        C_ = wo.shape[0]
        wo[[0, 7, C_ - 1]] *= 30
        w2[:, [3, 100, 4 * C_ - 1]] *= 30
        n = f"unet.layer{blk + 1}"
        unet.model.set_param(_param_index(unet.model, n + ".layer10.kernel"), wo)
        unet.model.set_param(_param_index(unet.model, n + ".layer9.weight"), w2)
        unet.model.prepare()
        C_, wf, bf = _fold(unet.model, blk)
        _check_fold(wf, bf, wo, bo, w2, b2)
        rng = np.random.default_rng(SEED)
        lat, cond, temb = (rng.standard_normal(s).astype(np.float32) for s in ((1, 4, 16, 16), (1, 77, 768), (1, 320)))
        recs = _recorded(ctx, lambda: unet.forward(lat, cond, temb))
        folds = [d for d in recs if not d[G.GD["CONV"]] and d[G.GD["N"]] == C_ and d[G.GD["K"]] == 5 * C_ and d[G.GD["K0"]] == 4 * C_]
        assert folds, "no fold GEMM recorded"
        for d in folds[:1]:
            ops = G.make_operands(d, 9)
            assert ops["W"].size == C_ * 5 * C_
            ops["W"] = np.ascontiguousarray(wf).ravel()
            rc, outs, info = run(ctx, d, ops, -1)
            assert rc == 0 and info[2] == 0
            rows = G.sample_rows(d, 3)
            assert G.check(d, ops, outs, rows) == []
    finally:
        unet.model.close()


def test_a_fold_that_leaves_fp16_is_reported(ctx, tsd_mod, unet_params):
    unet = tsd_mod.Diffusion(seed=SEED, ctx=ctx)
    try:
        unet.model.prepare()
        blk = 0
        while replay.lib().tsd_debug_model_fold(unet.model.h, blk, None, None) == 0:
            blk += 1
        assert replay.lib().tsd_debug_model_fold(unet.model.h, blk, None, None) > 0, "no attention block folds"
        wo, _, w2, _ = (np.array(x, np.float32) for x in _fold_params(unet_params, blk))
        n = f"unet.layer{blk + 1}"
        unet.model.set_param(_param_index(unet.model, n + ".layer10.kernel"), np.full_like(wo, 16.0))
        unet.model.set_param(_param_index(unet.model, n + ".layer9.weight"), np.full_like(w2, 16.0))  # 640 * 256 > 65504
        assert replay.lib().tsd_model_prepare(unet.model.h) == -7, "a folded weight outside fp16 was accepted"
        assert "not finite" in replay.lib().tsd_last_error().decode()
    finally:
        unet.model.close()
