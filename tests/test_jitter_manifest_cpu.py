"""CPU: the manifest of replay cases the jitter build is held to the shipped bits on (tests/jitter_manifest.py) - its names, what its
parts reach (every forced tile configuration and split-K way count with the plan the host makes for each, all five flash-attention
instances and four row-softmax kernels, every k_small_linear instance and pass count), the digest function, and - in the compiler's
listings of both builds - that every kernel the manifest counts on carries a jitter point in the jitter build and none in the shipped one."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import attn_ref as A
import elem_ref as E
import gemm_ref as G
import jitter_manifest as M
import replay

_i64p = C.POINTER(C.c_int64)


def test_names_are_unique_and_every_family_is_there():
    cases = M.manifest()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert [f for f in M.FAMILIES if not M.family(f)] == []
    assert all(c.name.startswith(c.family + "/") for c in cases)
    for fam in M.FAMILIES:   # the slices of a family are a partition of it, in order
        for n in (1, 4, 7):
            parts = [M.select(fam, (i, n)) for i in range(n)]
            assert sorted((c.name for p in parts for c in p)) == sorted(c.name for c in M.family(fam))


def test_the_other_families_are_the_tables_of_the_fp64_tests():
    import chain_ref as R
    import norm_ref as N
    assert [c.name for c in M.family("chain")] == ["chain/" + n for n in R.NAMES]
    assert len(M.family("attn")) == len(A.sweep()) + len(A.softmax_sweep())
    assert len(M.family("norm")) == len(N.sweep()) + len(N.ln_sweep())
    assert {N.F(c.desc, "C") for c in M.family("norm") if N.mode_of(c.desc) == "LAYERNORM"} == {320, 640, 1280, 8, 64, 768, 1024, 2048}
    assert len(M.family("lora")) == 3 + 12
    assert [c.name for c in M.family("model")] == ["model/unet_cfg_b2_l16", "model/unet_b3_l24", "model/decoder_l16", "model/encoder_128px",
                                                   "model/clip_b2"]


# ---- gemm ---------------------------------------------------------------------------------------------------------------------------
def _plan(case):
    d = np.ascontiguousarray(case.desc, np.int64)
    p = np.zeros(G.GP["COUNT"], np.int64)
    if case.ctx_opt:
        os.environ[case.ctx_opt[0]] = case.ctx_opt[1]
    try:
        rc = replay.lib().tsd_debug_gemm_plan(None, d.ctypes.data_as(_i64p), len(d), case.extra, p.ctypes.data_as(_i64p))
    finally:
        if case.ctx_opt:
            del os.environ[case.ctx_opt[0]]
    return rc, p


def test_gemm_part_reaches_every_configuration_and_way_count_and_plans_as_expected():
    cases = M.family("gemm")
    forced = [c for c in cases if c.extra >= 0]
    sweep = G._sweep_cases()
    assert len(forced) == sum(len([c for c in cfgs if not (c == 30 and int(d[G.GD["N"]]) % 160)]) for _, d, cfgs in sweep)
    assert {c.extra for c in forced} == set(G.N160 + G.N128 + G.THIN + (30, 32))
    assert all(c.recipe == ("gemm", c.extra) for c in forced)                      # the seed of the fp64 sweep: the configuration
    want_ways = {f"gemm/split/{name}": ways for name, _, ways in G.SPLITS}
    assert set(want_ways.values()) == {2, 4, 8}
    names = {c.name: c for c in cases}
    assert set(want_ways) <= set(names) and "gemm/vt_tail" in names
    assert names["gemm/optin_256_row_split"].ctx_opt == ("TSD_GEMM_SK256", "3")
    assert [c.name for c in cases if c.ctx_opt] == ["gemm/optin_256_row_split"]
    refused = 0
    for c in cases:
        rc, p = _plan(c)
        assert rc == 0, f"{c.name}: plan status {rc}: {replay.lib().tsd_last_error().decode()}"
        cfg, ways = int(p[G.GP["CFG"]]), int(p[G.GP["WAYS"]])
        if c.extra >= 0:
            assert (cfg, ways) == (c.extra, 1), f"{c.name}: planned ({cfg}, {ways})"
        elif c.name in want_ways:
            assert ways == want_ways[c.name], f"{c.name}: planned {ways} slices"
        elif c.name == "gemm/optin_256_row_split":
            assert (cfg, ways) == (51, 4)
        else:
            assert c.name == "gemm/vt_tail" and ways == 1
        if int(c.desc[G.GD["EPI"]]) & G.EPI["GNSTATS"]:   # the launch refuses exactly the tiles whose wave columns hold no whole groups
            cpg = int(c.desc[G.GD["N"]]) // int(c.desc[G.GD["GN_GROUPS"]])
            emits = int(p[G.GP["GN_NSLAB"]]) > 0
            assert emits == (G.BNW[c.extra] % cpg == 0), f"{c.name}: the plan emits {int(p[G.GP['GN_NSLAB']])} slabs"
            refused += not emits
    assert refused > 0          # pairs the kernel refuses stay in the manifest (the GPU test compares their status)


# ---- attn / elem --------------------------------------------------------------------------------------------------------------------
def test_attn_part_reaches_all_five_flash_instances_and_four_softmax_kernels():
    attn = [c for c in M.family("attn") if c.recipe[0] == "attn"]
    soft = [c for c in M.family("attn") if c.recipe[0] == "softmax"]
    assert {A.plan(c.desc)["KERNEL"] for c in attn} == {A.AK[k] for k in ("40_1", "40_2", "40_8W", "80", "160")}
    assert {A.softmax_kernel(c.desc) for c in soft} == set(A.SOFTMAX_KERNEL.values()) and len(A.SOFTMAX_KERNEL) == 4
    assert all(c.recipe == ("attn", kind, 7) for c, (_, _, kind) in zip(attn, A.sweep()))


def test_elem_part_reaches_every_nb_instance_and_both_pass_counts():
    expect = {"elem/" + name: e for name, d, _, e in E.sweep() if E.mode_of(d) == "SMALL_LINEAR"}
    cases = M.family("elem")
    assert [c.name for c in cases] == list(expect)
    assert {expect[c.name]["NB"] for c in cases} == {1, 2, 4, 8, 16}
    assert {expect[c.name]["PASSES"] for c in cases} == {1, 2}
    assert all(E.mode_of(c.desc) == "SMALL_LINEAR" for c in cases)


# ---- the digest -----------------------------------------------------------------------------------------------------------------------
PINNED = {
    "gemm": "7d63c886c4d4617592e6f26b3dbd8707e42bc722",
    "attn": "ee08c2bc6d87eff39faf219a44242b5bf34d954b",
    "chain": "ce6fee021b8a04531e3629dd713dae006dc2fef8",
    "norm": "7253c26c30a825d47bd530540771cff70022af91",
    "elem": "466f263a81fe4b8be6ba997899e1814ef82189e9",
    "lora": "28f111d7f00a1689dd58cfbed59cd2bcc801178d",
    "model": "3b98c1eda1f00b12e7ef0a04efb8aea6c40cbae9",
}


def _synthetic(fam):
    return [np.arange(6, dtype=np.float16), np.array([1.5, -2.0], np.float32)], list(range(1, len(M.INFO_FIELDS[fam]) + 1))


@pytest.mark.parametrize("fam", M.FAMILIES)
def test_digest_is_stable_and_moves_with_one_bit_or_one_field(fam):
    outs, info = _synthetic(fam)
    base = M.digest(fam, outs, info)
    assert base == PINNED[fam]
    by_hand = hashlib.sha1(fam.encode() + outs[0].tobytes() + outs[1].tobytes() + b"".join(int(v).to_bytes(8, "little") for v in info))
    assert base == by_hand.hexdigest()
    for slot in range(2):
        flipped = [o.copy() for o in outs]
        flipped[slot].view(np.uint8)[-1] ^= 1
        assert M.digest(fam, flipped, info) != base
    for i in range(len(info)):
        moved = list(info)
        moved[i] += 1
        assert M.digest(fam, outs, moved) != base
    assert len({M.digest(f, outs, info) for f in M.FAMILIES if len(M.INFO_FIELDS[f]) == len(info)}) == \
        len([f for f in M.FAMILIES if len(M.INFO_FIELDS[f]) == len(info)])


def test_info_fields_are_what_the_fp64_tests_assert_and_none_is_a_clock():
    import chain_ref as R
    import norm_ref as N
    assert M.INFO_FIELDS["gemm"] == (0, 1, 2)
    assert sorted(M.INFO_FIELDS["attn"]) == sorted(v for k, v in A.AI.items() if k != "COUNT")
    assert sorted(M.INFO_FIELDS["elem"]) == sorted(v for k, v in E.EI.items() if k != "COUNT")
    assert sorted(M.INFO_FIELDS["chain"]) == sorted(v for k, v in R.CI.items() if k != "COUNT")
    names = [k for k in list(A.AI) + list(E.EI) + list(R.CI) + list(N.NI)]
    assert not [k for k in names if any(w in k for w in ("TICK", "TIME", "CLOCK"))], names
    assert M.info_of("elem", np.arange(10, 20)) == [10 + E.EI[k] for k in ("NB", "PASSES", "NONFINITE", "CHANGED")]


# ---- the jitter points, in the listings ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem,kernel", M.JITTER_KERNELS, ids=[k for _, k in M.JITTER_KERNELS])
def test_kernel_carries_a_jitter_point_in_the_jitter_build_only(stem, kernel):
    jit, shipped = M.listing("build_jitter", stem), M.listing("build", stem)
    if not os.path.isdir(os.path.dirname(jit)):
        pytest.skip("csrc/build_jitter/ is not there (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    assert os.path.exists(jit) and os.path.exists(shipped), (jit, shipped)
    perturbed = {f: n for f, n in M.points_per_function(jit).items() if M.kernel_of(f) == kernel}
    plain = {f: n for f, n in M.points_per_function(shipped).items() if M.kernel_of(f) == kernel}
    assert perturbed and set(perturbed) == set(plain), f"{kernel}: the two builds do not have the same instantiations"
    for f, (sleeps, clocks) in perturbed.items():
        assert sleeps >= 1 and clocks >= 1, f"{f}: no jitter point in the jitter listing ({sleeps} s_sleep, {clocks} s_memtime)"
        assert sleeps > plain[f][0], f"{f}: the jitter listing sleeps no more often than the shipped one"
    for f, (sleeps, clocks) in plain.items():   # the shipped listing reads no clock, and sleeps only where the source itself waits
        assert clocks == 0, f"{f}: the shipped listing reads the clock"
        assert sleeps == 0 or kernel in M.SHIPPED_SLEEPS, f"{f}: the shipped listing sleeps"


def test_families_of_the_manifest_are_covered_by_the_kernel_list():
    kernels = {k for _, k in M.JITTER_KERNELS}
    assert {"gemm_kernel", "flash_attn_kernel", "flash_attn8_kernel", "attn_chain_kernel", "k_cfg_moments", "k_gn_partial", "k_gn_prereduce",
            "k_gn_apply", "k_softmax_rows", "k_softmax_rows_h8", "k_small_linear", "k_lora_merge"} == kernels
    assert M.kernel_of("_Z12k_gn_partial3GnK") == "k_gn_partial" and M.kernel_of("main") == "main"
