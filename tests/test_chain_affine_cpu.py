"""No GPU: tsd_debug_chain_run_affine is declared, exported and bound and sizes without a context; chain_affine_ref with the identity
affine, the reference's rstd and the tanh GELU is chain_ref, exactly."""
import numpy as np
import pytest

import chain_affine_ref as A
import chain_ref as R
import replay


def test_entry_is_declared_exported_bound_and_sizes_without_a_context():
    from tsd import _lib
    assert "tsd_debug_chain_run_affine" in _lib.declared_symbols()
    L, d = replay.lib(), R.tail_desc(2, 128, gn=1)
    ext, dd = np.zeros(64, np.int64), np.ascontiguousarray(d)
    rc = L.tsd_debug_chain_run_affine(None, replay._p(dd), len(dd), None, None, replay._p(ext), None, 0, None, 0)
    assert rc == 0 and {s: int(ext[R.CO[s]]) for s in R.extents(d)} == R.extents(d)
    assert L.tsd_debug_chain_run_affine(None, replay._p(dd), len(dd), None, None, replay._p(ext), None, 0, None, 2) != 0   # unknown flag


@pytest.mark.parametrize("name", ["tail/B1_S64", "head/B1_S64"])
def test_identity_affine_with_tanh_is_chain_ref(name):
    d, _, ops, ref, emu = R.case(name)
    got, (eo, e32) = A.reference(d, ops, A.IDENTITY, erf=False, torch=False), A.emulate(d, ops, A.IDENTITY, erf=False, torch=False)
    assert all(np.array_equal(got[s], ref[s]) for s in ref)
    assert all(np.array_equal(eo[s].view(np.uint8), emu[0][s].view(np.uint8)) for s in eo) and all(np.array_equal(e32[s], emu[1][s]) for s in e32)
    other = A.reference(d, ops, A.draw_affine(1))
    assert all(np.abs(other[s] - ref[s]).max() > 1e-2 for s in ref)                          # ... and the terms act
