"""No GPU: the surface of shared self attention - symbols, the version-4 fields, contract rows - and that the inputs of
tests/test_gpu_attnshare.py are well conditioned on the gathered problems.  (A model lives on a device: the setter's refusals are in that file.)"""
import json
import os

import attn64_ref as R
import attn_ref as A
import attnshare_ref as S
import replay

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd")
NEW_ENTRIES = ("tsd_model_set_attn_share", "tsd_model_attn_share")


def test_symbols_enum_values_contract_rows_and_well_conditioned_inputs(tsd_mod):
    lib, shim = tsd_mod._lib.lib(), open(os.path.join(PKG, "mojo_shim", "tsd_ffi.mojo")).read()
    for n in NEW_ENTRIES:
        assert n in tsd_mod._lib.declared_symbols() and hasattr(lib, n) and getattr(lib, n).argtypes and f'"{n}"' in shim, n
        assert getattr(lib, n)(None, None, 0, None, *([0] if "set" in n else [None])) == tsd_mod._lib.TSD_E_ARG      # no model
    assert all(hasattr(tsd_mod.Diffusion, n) for n in ("set_attn_share", "attn_share", "clear_attn_share"))
    txt = replay.header()              # the existing enum values are what they were and the table follows version 3's fields
    assert A.AD["COUNT"] == 24 and replay.version(txt, "TSD_AD_VERSION_4") == 4
    assert "enum tsd_attn_desc_field_v4 { TSD_AD4_SHARE_N = TSD_AD3_COUNT, TSD_AD4_SHARE_0, TSD_AD4_COUNT = TSD_AD4_SHARE_0 + 8 }" in txt
    rows = json.load(open(os.path.join(PKG, "csrc", "isa_contract.json")))["kernels_attn"]
    new = {k: r["regs"] for k, r in rows.items() if "flash_attn_share_kernel" in k}
    assert len(new) == 5 and all("scratch=0" in r and "vgpr_spill=0" in r for r in new.values()), new
    for i, (hd, _, _, table, _) in enumerate(S.CASES):
        base, _, ops = S.case(i)
        assert all((R if hd == 64 else A).well_conditioned(*S.gathered(base, ops, b, t)) for b, t in enumerate(table)), S.IDS[i]
