"""CPU: the e4m3 reference of the FP8 feed-forward (tests/fp8_ref.py) against itself and the specification, and the ABI's new names."""
import numpy as np

import fp8_ref as R


def test_encode_and_decode_round_trip_every_finite_code():
    codes = np.array([c for c in range(256) if c & 127 != 127], np.uint8)
    assert np.array_equal(R.e4m3_encode(R.E4M3[codes].astype(np.float32)), codes)   # -0 (0x80) included
    assert R.E4M3[0x7E] == 448.0 and R.E4M3[0x01] == 2.0 ** -9 and R.E4M3[0x08] == 2.0 ** -6 and np.isnan(R.E4M3[[0x7F, 0xFF]]).all()


def test_quantiser_rounds_ties_to_even_and_flags_non_finite_rows():
    x = np.zeros((4, 128), np.float16)
    x[0, :6] = [448, 17, 19, -17, 3 * 2.0 ** -10, 5 * 2.0 ** -10]   # amax = 448: inv = 1; midpoints of the 16 .. 32 and subnormal grids
    x[2, 5] = np.inf
    x[3, :2] = [65504, -32752]
    q, s = R.quant_rows(x)
    assert list(R.E4M3[q[0, :6]]) == [448, 16, 20, -16, 2 * 2.0 ** -9, 2 * 2.0 ** -9] and s[0] == 1
    assert s[1] == 1 and not q[1].any() and np.isnan(s[2]) and not q[2].any()
    assert list(q[3, :2]) == [0x7E, 0xF6] and s[3] == np.float32(65504) / np.float32(448)
    y = R.fake_quant_linear(x[:1], x[:1])
    assert y[0, 0] == 448.0 ** 2 + 16 ** 2 + 20 ** 2 + 16 ** 2 + 2 * (2 * 2.0 ** -9) ** 2


def test_abi_names_exist_and_a_null_model_is_refused():
    import tsd
    lib = tsd._lib.lib()
    names = ("tsd_model_set_ff_fp8", "tsd_model_ff_fp8", "tsd_quant_rows_e4m3", "tsd_fp8_gemm_f16", "tsd_linear_fp8_f32")
    assert all(hasattr(lib, n) and n in tsd._lib.declared_symbols() for n in names)
    assert lib.tsd_model_set_ff_fp8(None, 1) == tsd._lib.TSD_E_ARG and lib.tsd_model_ff_fp8(None) == tsd._lib.TSD_E_ARG
    assert all(hasattr(tsd, n) for n in ("quant_rows_e4m3", "fp8_gemm", "linear_fp8")) and hasattr(tsd.Diffusion, "set_ff_fp8") and hasattr(tsd.ControlNet, "set_ff_fp8")
