"""No GPU: the surface of windowed self attention - symbols, enum values, the sizing mode on version-3 descriptors, refusals, contract rows."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import attn_ref as A
import replay

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd")


def win_desc(B, H, hd, win, gh, gw):
    d = np.concatenate([A.attn_desc(B, H, hd, gh * gw, gh * gw), np.array([win, gh, gw], np.int64)])     # TSD_AD3_WIN, _GRID_H, _GRID_W
    d[A.AD["VERSION"]] = 3
    return d


def test_symbols_enum_values_and_contract_rows(tsd_mod):
    lib, shim = tsd_mod._lib.lib(), open(os.path.join(PKG, "mojo_shim", "tsd_ffi.mojo")).read()
    for n in ("tsd_model_set_attn_window", "tsd_model_attn_window"):
        assert n in tsd_mod._lib.declared_symbols() and hasattr(lib, n) and getattr(lib, n).argtypes and f'"{n}"' in shim, n
    assert hasattr(tsd_mod.Diffusion, "set_attn_window") and hasattr(tsd_mod.ControlNet, "set_attn_window")
    txt = replay.header()              # the existing enum values are what they were and the window fields follow them
    assert A.AD["COUNT"] == 24 and list(A.AD)[-2] == "ZERO_TO" and replay.version(txt, "TSD_AD_VERSION_3") == 3
    assert A.AK == {"NONE": 0, "40_1": 1, "40_2": 2, "40_8W": 3, "80": 4, "160": 5, "64": 6}
    assert "enum tsd_attn_desc_field_v3 { TSD_AD3_WIN = TSD_AD_COUNT, TSD_AD3_GRID_H, TSD_AD3_GRID_W, TSD_AD3_COUNT }" in txt
    rows = json.load(open(os.path.join(PKG, "csrc", "isa_contract.json")))["kernels_attn"]
    new = {k: r["regs"] for k, r in rows.items() if "flash_attn_win_kernel" in k}
    assert len(new) == 5 and all("scratch=0" in r and "vgpr_spill=0" in r for r in new.values()), new


@pytest.mark.parametrize("case, kernel", [((1, 8, 40, 32, 32, 64), "40_2"), ((2, 8, 40, 8, 16, 24), "40_1")])
def test_sizing_mode_plans_a_version_3_descriptor_on_the_windows_shape(tsd_mod, case, kernel):
    info = np.zeros(8, np.int64)
    assert replay.size("tsd_debug_attn_run", win_desc(*case), info=info)[0] == 0
    assert info[A.AI["KERNEL"]] == A.AK[kernel] and info[A.AI["DIAG"]] == 1


def test_refusals(tsd_mod):
    E, good = tsd_mod._lib, win_desc(1, 8, 40, 8, 16, 24)
    for field, value in ((24, 12), (24, 256), (25, 15), (26, 0)):           # a side outside the list, a grid that is not Sq
        bad = np.where(np.arange(good.size) == field, value, good)
        assert replay.size("tsd_debug_attn_run", bad)[0] == E.TSD_E_ARG, (field, value)
    assert replay.size("tsd_debug_attn_run", good, n=A.COUNT)[0] == E.TSD_E_ARG        # version 3 needs its three fields
    assert E.lib().tsd_model_set_attn_window(None, (C.c_int * 4)(8, 0, 0, 0)) == E.TSD_E_ARG
    assert E.lib().tsd_model_attn_window(None, None) == E.TSD_E_ARG
