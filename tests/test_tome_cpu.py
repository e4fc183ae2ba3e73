"""No GPU: token merging's symbols (header, _lib.py, shim), contract rows and device-free refusals; tome_ref's hash and partition by hand."""
import ctypes as C
import json
import os

import numpy as np

import tome_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stable-diffusion.mojo_amd")
SYMBOLS = ("tsd_model_set_token_merge", "tsd_model_token_merge", "tsd_token_merge_plan_f16", "tsd_token_merge_rows_f16",
           "tsd_token_unmerge_rows_f16", "tsd_debug_token_merge_record", "tsd_debug_token_merge_recorded")


def test_symbols_contract_rows_and_refusals_without_a_device(tsd_mod):
    E, header = tsd_mod._lib, open(os.path.join(ROOT, "include", "tsd.h")).read()
    shim = open(os.path.join(PKG, "mojo_shim", "tsd_ffi.mojo")).read()
    for n in SYMBOLS:
        assert n in E.declared_symbols() and getattr(E.lib(), n).argtypes and f"int {n}(" in header, n
        assert n.startswith("tsd_debug") or f'"{n}"' in shim, n
    for cls in (tsd_mod.Diffusion, tsd_mod.ControlNet):
        assert hasattr(cls, "set_token_merge") and isinstance(cls.token_merge, property)
    rows = json.load(open(os.path.join(PKG, "csrc", "isa_contract.json")))["kernels_tome"]
    assert {k.split("k_tome_")[1][:5] for k in rows} == {"match", "selec", "merge", "unmer"} and len(rows) == 5   # match has two instances
    assert all("scratch=0" in r["regs"] and "vgpr_spill=0" in r["regs"] and "counted=0" in r["waits"] for r in rows.values()), rows
    assert E.lib().tsd_model_set_token_merge(None, (C.c_float * 4)(0.5, 0, 0, 0), 0) == E.TSD_E_ARG
    assert E.lib().tsd_model_token_merge(None, None, None) == E.TSD_E_ARG
    assert E.lib().tsd_token_merge_plan_f16(None, None, 1, 8, 8, 320, 0.5, 0, None, None, None, None, None) == E.TSD_E_ARG


def test_hash_and_partition_against_hand_written_answers():
    assert T.tome_hash(1, 0) == 0x514E28B7 and T.tome_hash(0, 0) == 0       # murmur3's finaliser of 1
    dst, src = T.partition(4, 4, 0)                                         # seed 0: the top-left token of every cell
    assert dst.tolist() == [0, 2, 8, 10] and src.tolist() == [1, 4, 5, 3, 6, 7, 9, 12, 13, 11, 14, 15]
    dst, src = T.partition(4, 4, 5)
    cells = [[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 12, 13], [10, 11, 14, 15]]
    assert dst.tolist() == [cells[c][T.tome_hash(5, c) & 3] for c in range(4)]
    assert all(sorted(src[3 * c:3 * c + 3].tolist() + [dst[c]]) == cells[c] and src[3 * c] < src[3 * c + 1] < src[3 * c + 2] for c in range(4))
    assert len({T.tome_hash(5, c) & 3 for c in range(64)}) == 4             # every position is taken somewhere
    assert [T.merged_count(r, 64) for r in (0.0, 0.12, 0.13, 0.5, 0.75)] == [0, 0, 8, 32, 48]
    v = np.array([.1, .9, .9, .2, .9, .3, 0, 0, 0, 0, 0, 0], np.float32).repeat(4)     # the eight largest: sources 4 .. 11, all into destination 0
    row_of, start, members = T.plan(v, np.zeros(48, np.int64), 8, 8, 8, 0)
    assert len(start) == 57 and start[-1] == 64 and sorted(members.tolist()) == list(range(64)) and np.bincount(row_of)[40] == 9
