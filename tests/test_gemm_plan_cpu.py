"""The host plan of a GEMM / conv3x3 launch (csrc/gemm_plan.cpp) asked through tsd_debug_gemm_plan with no context and no device:
pinned to what the parent library launched on the GPU (tests/golden/gemm_plans.json), held to batch invariance of the summation
tree over B = 1..16 for every layer class of that file, and to the tile table for forced configurations."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gemm_ref as G
import replay
from gemm_ref import GP, N128, N160, THIN

_i64p = C.POINTER(C.c_int64)
E_ARG = -1
with open(os.path.join(replay.ROOT, "tests", "golden", "gemm_plans.json")) as _f:
    GOLDEN = json.load(_f)
assert GOLDEN["fields"] == sorted(G.GD, key=G.GD.get), "the descriptor layout moved: record tests/golden/gemm_plans.json again"
RECORDED = [np.array(d, np.int64) for d in GOLDEN["descriptors"]]
UPS_FOLD_IDS = {0, 1, 5, 6, 7, 51}  # csrc/gemm_tiles.h UF_Y


@pytest.fixture(autouse=True)
def default_options(monkeypatch):
    """A NULL context plans under the options of the environment: the defaults."""
    for k in list(os.environ):
        if k.startswith("TSD_") and k != "TSD_LIB":
            monkeypatch.delenv(k)


def plan(d, cfg=-1):
    """(status, plan fields) of descriptor d without a context."""
    d = np.ascontiguousarray(d, np.int64)
    out = np.full(GP["COUNT"], -99, np.int64)
    rc = replay.lib().tsd_debug_gemm_plan(None, d.ctypes.data_as(_i64p), len(d), cfg, out.ctypes.data_as(_i64p))
    return rc, {k: int(out[v]) for k, v in GP.items() if k != "COUNT"}


def _g(d, k):
    return int(d[G.GD[k]])


def test_the_plan_is_what_the_parent_library_launched():
    assert len(RECORDED) > 250 and len(GOLDEN["parent_commit"]) == 40
    seen = set()
    for d in RECORDED:
        rc, p = plan(d)
        what = f"M {_g(d, 'M')} N {_g(d, 'N')} K {_g(d, 'K')} conv {_g(d, 'CONV')} rps {_g(d, 'RPS_HINT')}"
        assert rc == 0, f"{what}: {replay.lib().tsd_last_error().decode()}"
        assert (p["CFG"], p["WAYS"]) == (_g(d, "CFG"), _g(d, "WAYS")), f"{what}: planned {p}"
        if _g(d, "EPI") & G.EPI["GNSTATS"]:
            assert p["GN_NSLAB"] == _g(d, "GN_NSLAB") > 0, f"{what}: statistics slabs {p['GN_NSLAB']}"
        fold = _g(d, "CONV") and _g(d, "UPS") == 2
        assert p["K"] == (4 * _g(d, "CIN") if fold else _g(d, "K")) and (p["VARIANT"] == 3) == bool(fold), f"{what}: {p}"
        assert p["WS_FLOATS"] == ((p["WAYS"] - 1) * -(-_g(d, "M") // p["BM"]) * -(-_g(d, "N") // p["BN"]) * p["BM"] * p["BN"])
        seen.add((p["CFG"], p["WAYS"] > 1, p["VARIANT"]))
    assert {c for c, _, _ in seen} >= {0, 2, 5, 7, 24, 47, 51, 53, 54} and {v for _, _, v in seen} == {0, 2, 3}, seen
    assert any(s for _, s, _ in seen)


# ---- batch invariance of the summation tree -----------------------------------------------------------------------------------
def _rows_per_sample(d):
    """Rows of one sample: the image for a convolution, else what the graph told the launcher; a launch that carries neither
    (the dispatcher never splits it) is taken whole."""
    return _g(d, "HO") * _g(d, "WO") if _g(d, "CONV") else (_g(d, "RPS_HINT") or _g(d, "M"))


def _layer_classes():
    out = {}
    for d in RECORDED:
        c = d.copy()
        c[G.GD["M"]] = _rows_per_sample(d)
        c[G.GD["CFG"]], c[G.GD["WAYS"]] = -1, 0
        out.setdefault(tuple(int(x) for x in c), c)
    return list(out.values())


# rows per sample 64, N = 10240, K = 1280 - the first GEGLU linear of a C = 1280 attention block at an 8x8 level: 64-row tiles give 64
# tile columns, and from B = 9 on the 9+ tile rows exceed 2 * splitk_tiles, so the launch splits K in two for B = 1..8 and not at all
# for B = 9..16 (csrc/gemm_plan.cpp splitk_plan).  Known, pinned here, to be fixed by a change of its own (it moves bits at some batches).
def _varies_with_the_batch(c):
    return not _g(c, "CONV") and (_rows_per_sample(c), _g(c, "N"), _g(c, "K")) == (64, 10240, 1280)


LAYERS = _layer_classes()


def _layer_id(c):
    return f"{'conv' if _g(c, 'CONV') else 'dense'}-rps{_g(c, 'M')}-n{_g(c, 'N')}-k{_g(c, 'K')}-e{_g(c, 'EPI')}-u{_g(c, 'UPS')}-b{_g(c, 'SK_BIG')}"


def test_the_known_batch_dependent_layer_is_among_the_recorded_ones():
    assert sum(1 for c in LAYERS if _varies_with_the_batch(c)) >= 1 and len(LAYERS) > 100


@pytest.mark.parametrize("layer", [
    pytest.param(c, id=f"{i}-{_layer_id(c)}",
                 marks=[pytest.mark.xfail(strict=True, reason="rps 64, N 10240, K 1280: split-K by 2 for B <= 8, none for B >= 9")]
                 if _varies_with_the_batch(c) else []) for i, c in enumerate(LAYERS)])
def test_ways_variant_and_executed_k_do_not_depend_on_the_batch(layer):
    rps, tree = _g(layer, "M"), {}
    for B in range(1, 17):
        d = layer.copy()
        d[G.GD["M"]] = B * rps
        rc, p = plan(d)
        assert rc == 0, f"B {B}: {replay.lib().tsd_last_error().decode()}"
        tree[B] = (p["WAYS"], p["VARIANT"], p["K"])
    assert all(t == tree[1] for t in tree.values()), f"(ways, variant, executed K) per batch size: {tree}"


# ---- forced configurations --------------------------------------------------------------------------------------------------------
def _forced_desc(cfg):
    """A launch the dispatcher would split (rows per sample 64, K = 8192) in the column family of the tile; a thin one for THIN."""
    if cfg in THIN:
        return G.conv_desc(B=2, Hs=9, Ws=7, Cin=128, N=8, epi=G.EPI["BIAS_N"])
    return G.dense_desc(M=256, N=1280 if cfg in N160 else 1024, K=8192, epi=G.EPI["BIAS_N"], rps_hint=64)


# LDS of the plain tiles, NS * (BM + BN) * 128 bytes, worked out by hand from the table's (BM x BN, ring slots)
LDS_KIB = {0: 72, 1: 56, 2: 64, 3: 48, 4: 36, 24: 40, 5: 108, 6: 112, 7: 84, 8: 96, 9: 96, 10: 72, 11: 156, 13: 144, 51: 156, 54: 108}


@pytest.mark.parametrize("cfg", N160 + N128 + THIN)
def test_a_forced_configuration_is_planned_as_itself_unsplit(cfg):
    d = _forced_desc(cfg)
    if cfg not in THIN:
        assert plan(d)[1]["WAYS"] == 8
    rc, p = plan(d, cfg)
    assert rc == 0 and (p["CFG"], p["WAYS"], p["WS_FLOATS"]) == (cfg, 1, 0), p
    assert p["BN"] == (16 if cfg in THIN else 160 if cfg in N160 else 128) and p["BM"] % p["BMW"] == 0 and p["BN"] % p["BNW"] == 0
    if cfg in LDS_KIB:
        assert p["LDS_BYTES"] == LDS_KIB[cfg] * 1024, p


@pytest.mark.parametrize("cfg", (22, 23, 31, 33, 52, 56, 63, 64, 1000))
def test_an_id_outside_the_tile_table_is_refused(cfg):
    for d in (_forced_desc(0), G.conv_desc(B=1, Hs=4, Ws=64, Cin=64, N=256, epi=G.EPI["BIAS_N"])):
        rc, p = plan(d, cfg)
        assert rc == E_ARG and set(p.values()) == {-99}, (rc, p)


def test_the_upsample_fold_is_refused_on_tiles_without_the_variant():
    folds = [d for d in RECORDED if _g(d, "CONV") and _g(d, "UPS") == 2]
    assert folds
    for d in folds:
        for cfg in N160 + N128 + THIN + (30, 32):
            rc, p = plan(d, cfg)
            if cfg in UPS_FOLD_IDS:
                assert rc == 0 and (p["CFG"], p["WAYS"], p["VARIANT"], p["K"]) == (cfg, 1, 3, 4 * _g(d, "CIN")), (cfg, p)
            else:
                assert rc == E_ARG, f"cfg {cfg} took an ups = 2 launch"
    bad = folds[0].copy()
    bad[G.GD["LDR"]] = _g(bad, "N")
    bad[G.GD["EPI"]] |= G.EPI["RESIDUAL"]  # a one-parity tile holds no residual rows: not foldable, whatever the tile
    assert plan(bad)[0] == E_ARG and plan(bad, 0)[0] == E_ARG


@pytest.mark.parametrize("cfg,N,lds", [(30, 320, 75776), (32, 256, 67584)])
def test_a_forced_halo_tile_is_planned_as_the_halo_variant_of_its_plain_tile(cfg, N, lds):
    """LDS: the W ring (2 * BN * 128 bytes) plus two A buffers of BM / 8 + 1 KiB-rows each."""
    rc, p = plan(G.conv_desc(B=1, Hs=4, Ws=64, Cin=64, N=N, epi=G.EPI["BIAS_N"]), cfg)
    assert rc == 0 and (p["CFG"], p["WAYS"], p["VARIANT"], p["BM"], p["BMW"], p["LDS_BYTES"]) == (cfg, 1, 1, 128, 64, lds), p
    assert plan(G.conv_desc(B=1, Hs=8, Ws=128, Cin=64, N=N, stride=2, epi=G.EPI["BIAS_N"]), cfg)[0] == E_ARG
