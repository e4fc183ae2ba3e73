"""CPU: the MXFP4 reference (tests/mxfp4_ref.py) against the specification, and the ABI's new names."""
import numpy as np
import pytest

import mxfp4_ref as R


def test_abi_names_exist_and_mode_2_on_a_null_model_is_refused():
    import tsd
    lib = tsd._lib.lib()
    names = ("tsd_quant_weights_mxfp4", "tsd_mxfp4_gemm_f16")
    assert all(hasattr(lib, n) and n in tsd._lib.declared_symbols() for n in names)
    assert all(hasattr(tsd, n) for n in ("quant_weights_mxfp4", "mxfp4_gemm"))
    assert lib.tsd_model_set_ff_fp8(None, 2) == tsd._lib.TSD_E_ARG
    assert [tsd.fp8.ff_fp8_mode(v) for v in (False, None, True, "mxfp4")] == [0, 0, 1, 2]
    with pytest.raises(ValueError):
        tsd.fp8.ff_fp8_mode("fp4")


def test_e2m1_round_trips_its_fifteen_values_and_rounds_midpoints_to_even():
    codes = np.array([c for c in range(16) if c != 8], np.uint8)   # -0 (code 8) is not a sixteenth value
    assert np.array_equal(R.e2m1_encode(R.E2M1[codes]), codes)
    assert list(R.E2M1[R.e2m1_encode(R.MIDPOINTS)]) == [0, 1, 1, 2, 2, 4, 4] and list(R.E2M1[R.e2m1_encode(-R.MIDPOINTS)][1:]) == [-1, -1, -2, -2, -4, -4]
    assert list(R.E2M1[R.e2m1_encode([5.5, 7, 100, -9])]) == [6, 6, 6, -6]


@pytest.mark.parametrize("amax,byte,top", [(1.0, 125, 4), (7.0, 127, 6), (6.0, 127, 6), (65504.0, 140, 6), (2.0 ** -24, 101, 4), (3.0 * 2.0 ** -10, 116, 6)])
def test_block_scale_is_floor_log2_amax_minus_two(amax, byte, top):
    w = np.zeros((2, 32), np.float16)
    w[0, :2] = [amax, -amax]
    e, s = R.quant_weights(w)
    assert e.shape == (2, 64) and s.shape == (2, 4) and list(s[0]) == [byte, 127, 127, 127] and not e[1].any() and list(s[1]) == [127] * 4
    d = R.dequant(e, s)
    assert d[0, 0] == top * 2.0 ** (byte - 127) and d[0, 1] == -d[0, 0] and not d[0, 2:].any()
    assert abs(d[0, 0] - amax) <= amax / 4   # the top element: at worst 7 X -> 6 X and 5 X -> 4 X
    with pytest.raises(FloatingPointError):
        R.quant_weights(np.where(np.arange(32) == 5, np.inf, w))
