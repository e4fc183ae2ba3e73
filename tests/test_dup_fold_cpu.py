"""Host arithmetic of the duplicate-concat fold (UNet layer 10, TSD_FOLD_DUP): the two input-channel halves of an fp16 weight
[rows][taps][2 * half] are added exactly and rounded to fp16 ONCE, nearest-even.  Driven through `tsd_debug_dup_fold_host`, which
takes host pointers and touches no device.  The yardstick is numpy: fp16 -> float64 is exact, the float64 sum of two fp16 values is
exact (at most 40 binades + 11 bits < 53), and numpy's float64 -> float16 conversion rounds once, to nearest-even."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import tsd
    return tsd._lib.lib()


def fold(lib, w, half, ldo=None):
    """w: uint16 [rows][taps][ldw] -> (uint16 [rows][taps][ldo], number of non-finite sums)"""
    rows, taps, ldw = w.shape
    ldo = half if ldo is None else ldo
    w = np.ascontiguousarray(w)
    out = np.full((rows, taps, ldo), 0xAAAA, np.uint16)  # every element must be written
    bad = lib.tsd_debug_dup_fold_host(w.ctypes.data_as(C.c_void_p), rows, taps, ldw, half, out.ctypes.data_as(C.c_void_p), ldo)
    assert bad >= 0, bad
    return out, bad


def numpy_sum_bits(a16, b16):
    with np.errstate(over="ignore", invalid="ignore"):
        return (a16.astype(np.float64) + b16.astype(np.float64)).astype(np.float16).view(np.uint16)


def assert_same_bits(got, want):
    """bit for bit; a NaN must be a NaN (its payload is not part of the contract)"""
    nan = np.isnan(want.view(np.float16))
    assert np.array_equal(np.isnan(got.view(np.float16)), nan)
    assert np.array_equal(got[~nan], want[~nan]), np.argwhere((got != want) & ~nan)[:8]


def test_random_halves_equal_the_exact_sum_rounded_once(lib):
    """O = 8, 9 taps, I = 2 x 64.  Magnitudes spread over the whole fp16 range (subnormals included) and a block of exact bit patterns, so
    the halves are often many binades apart, which a float32 sum followed by a second rounding would get wrong."""
    r = np.random.default_rng(7)
    rows, taps, half = 8, 9, 64
    v = r.standard_normal((rows, taps, 2 * half)) * np.exp2(r.integers(-26, 16, (rows, taps, 2 * half)))
    with np.errstate(over="ignore"):
        w = v.astype(np.float16).view(np.uint16)  # a few land on inf: they pass through like any other value
    pat = r.integers(0, 0x7C00, (2, taps, 2 * half)).astype(np.uint16) | (r.integers(0, 2, (2, taps, 2 * half)).astype(np.uint16) << 15)
    w[:2] = pat  # finite patterns of every exponent, both signs
    got, bad = fold(lib, w, half)
    want = numpy_sum_bits(w[..., :half].view(np.float16), w[..., half:].view(np.float16))
    assert_same_bits(got, want)
    assert bad == int((~np.isfinite(want.view(np.float16))).sum())


def test_hand_made_rows(lib):
    h = lambda x: np.float16(x)  # noqa: E731
    sub = np.array([1], np.uint16).view(np.float16)[0]          # 2^-24, the smallest subnormal
    nan = np.array([0x7E00], np.uint16).view(np.float16)[0]
    pairs = [
        (h(2048.0), h(1.0)),          # 2049: tie between 2048 and 2050 -> even mantissa 2048
        (h(2050.0), h(1.0)),          # 2051: tie between 2050 and 2052 -> 2052
        (h(1024.0), h(0.5)),          # 1024.5: tie -> 1024
        (h(1026.0), h(0.5)),          # no tie above 1024: ulp 1 -> 1026.5 ties to 1026
        (h(1.0), sub),                # 1 + 2^-24: far below half an ulp -> 1
        (h(1.0), h(2.0 ** -11)),      # exactly half an ulp of 1 -> tie -> 1
        (h(1.0), h(2.0 ** -11 + 2.0 ** -21)),  # a little more than half an ulp -> 1 + 2^-10 (a float32 sum would be exact here too)
        (sub, h(6.1035e-05)),         # subnormal + smallest normal
        (sub, sub),                   # subnormal + subnormal = 2^-23
        (h(3.0), h(-3.0)),            # +x + -x = +0
        (h(-0.0), h(-0.0)),           # -0 + -0 = -0
        (h(32768.0), sub),            # 2^15 + 2^-24: 40 binades apart -> 2^15
        (h(40000.0), h(40000.0)),     # leaves fp16 -> inf
        (h(-40000.0), h(-40000.0)),   # -> -inf
        (h(65504.0), h(15.0)),        # 65519 < 65520: stays the largest finite value
        (h(65504.0), h(16.0)),        # 65520: tie to the even mantissa = overflow -> inf
        (nan, h(1.0)),                # a NaN passes through
        (h(1.0), nan),
        (h(np.inf), h(-np.inf)),      # inf - inf = NaN
        (h(np.inf), h(1.0)),          # inf stays inf
    ]
    half = 64
    a = np.zeros(half, np.float16)
    b = np.zeros(half, np.float16)
    for i, (x, y) in enumerate(pairs):
        a[i], b[i] = x, y
    w = np.concatenate([a, b]).view(np.uint16).reshape(1, 1, 2 * half)
    got, bad = fold(lib, w, half)
    want = numpy_sum_bits(a, b).reshape(1, 1, half)
    assert_same_bits(got, want)
    g = got.view(np.float16)[0, 0]
    assert g[0] == 2048.0 and g[1] == 2052.0 and g[2] == 1024.0 and g[4] == 1.0 and g[5] == 1.0 and g[6] == h(1.0 + 2.0 ** -10)
    assert got[0, 0, 9] == 0x0000 and got[0, 0, 10] == 0x8000          # +0 and -0 by their bits
    assert g[11] == 32768.0 and np.isposinf(g[12]) and np.isneginf(g[13]) and g[14] == 65504.0 and np.isposinf(g[15])
    assert np.isnan(g[16]) and np.isnan(g[17]) and np.isnan(g[18]) and np.isposinf(g[19])
    assert bad == 7   # three infinities from overflow, three NaNs, one inf passed through


def test_padding_rows_and_columns_stay_zero(lib):
    """Opad rows beyond O are zero in the packed weight and stay zero; output columns beyond cin/2 (an Ipad wider than the folded
    channel count) are written as zero; input columns beyond 2 * half are not read."""
    r = np.random.default_rng(8)
    O, Opad, taps, half, ldw, ldo = 5, 8, 9, 64, 2 * 64 + 64, 64 + 64
    w = np.zeros((Opad, taps, ldw), np.float16)
    w[:O, :, :2 * half] = r.standard_normal((O, taps, 2 * half)).astype(np.float16)
    w[:, :, 2 * half:] = np.float16(7.0)  # what a wider pitch may hold: must not leak into the result
    got, bad = fold(lib, w.view(np.uint16), half, ldo)
    assert bad == 0
    assert not got[O:].any(), "padding rows"
    assert not got[:, :, half:].any(), "padding columns"
    want = numpy_sum_bits(w[:O, :, :half], w[:O, :, half:2 * half])
    assert np.array_equal(got[:O, :, :half], want)


def test_bad_arguments_are_refused(lib):
    w = np.zeros((1, 1, 128), np.uint16)
    out = np.zeros((1, 1, 64), np.uint16)
    p, q = w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.tsd_debug_dup_fold_host(p, 1, 1, 127, 64, q, 64) < 0   # pitch narrower than the two halves
    assert lib.tsd_debug_dup_fold_host(p, 1, 1, 128, 64, q, 63) < 0   # output pitch narrower than one half
    assert lib.tsd_debug_dup_fold_host(None, 1, 1, 128, 64, q, 64) < 0
