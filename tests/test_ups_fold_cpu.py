"""Host arithmetic of the upsample fold (TSD_UPS_FOLD): `tsd_debug_ups_fold_host` turns 3x3 fp16 weights [O][3][3][Ipad] into the four
2x2 parity kernels [4][O][2][2][Ipad] - sums of up to four weights, exact in double, rounded to fp16 ONCE, nearest-even.  It takes host
pointers and touches no device.  The yardstick is numpy (tests/ups_fold_ref.py): fp16 -> float64 is exact, a sum of up to four fp16
values is an integer multiple of 2^-24 below 2^18 and so exact in float64, and numpy's float64 -> float16 conversion rounds once, to
nearest-even.  The second half holds the algebra itself in float64: with UNROUNDED folded weights the four phase convolutions ARE the
3x3 convolution of the nearest-upsampled image, borders included."""
import ctypes as C

import numpy as np
import pytest

import ups_fold_ref as U


@pytest.fixture(scope="module")
def lib():
    import tsd
    return tsd._lib.lib()


def fold(lib, w, Ipad, ldw=None):
    """w: uint16 [O][ldw] (ldw >= 9 Ipad) -> (uint16 [4][O][2][2][Ipad], number of non-finite sums)"""
    O = w.shape[0]
    w = np.ascontiguousarray(w.reshape(O, -1))
    ldw = w.shape[1] if ldw is None else ldw
    out = np.full((4, O, 2, 2, Ipad), 0xAAAA, np.uint16)  # every element must be written
    bad = lib.tsd_debug_ups_fold_host(w.ctypes.data_as(C.c_void_p), O, Ipad, ldw, out.ctypes.data_as(C.c_void_p))
    assert bad >= 0, bad
    return out, bad


def assert_same_bits(got, want):
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_random_weights_equal_the_exact_sums_rounded_once(lib):
    """Magnitudes spread over the whole fp16 range (subnormals included) plus rows of raw finite bit patterns: the terms of a sum are
    often many binades apart, which a float32 sum followed by a second rounding would get wrong."""
    r = np.random.default_rng(11)
    O, I = 6, 64
    v = r.standard_normal((O, 3, 3, I)) * np.exp2(r.integers(-26, 14, (O, 3, 3, I)))
    w = v.astype(np.float16).view(np.uint16)
    w[:2] = r.integers(0, 0x7400, (2, 3, 3, I)).astype(np.uint16) | (r.integers(0, 2, (2, 3, 3, I)).astype(np.uint16) << 15)
    got, bad = fold(lib, w, I)
    want = U.fold16(w.view(np.float16))
    assert_same_bits(got, want.view(np.uint16))
    assert bad == int((~np.isfinite(want)).sum())


def _one_group(vals):
    """a [1][3][3][64] weight whose channel c carries vals[c] (up to four terms) in kernel rows / columns {1, 2} x {1, 2}: the sum
    appears as parity 0, tap (1, 1)"""
    w = np.zeros((1, 3, 3, 64), np.float16)
    for c, t in enumerate(vals):
        for (kh, kw), x in zip(((1, 1), (1, 2), (2, 1), (2, 2)), t):
            w[0, kh, kw, c] = x
    return w


def test_hand_made_sums(lib):
    h = np.float16
    sub = np.array([1], np.uint16).view(np.float16)[0]   # 2^-24
    vals = [
        (h(2048.0), h(1.0)),                          # 2049: tie -> even mantissa 2048
        (h(2048.0), h(1.0), h(1.0), h(1.0)),          # 2051: tie between 2050 and 2052 -> 2052
        (h(1024.0), h(0.25), h(0.25)),                # 1024.5: tie -> 1024
        (h(1.0), h(2.0 ** -12), h(2.0 ** -12)),       # exactly half an ulp of 1 -> tie -> 1
        (h(1.0), h(2.0 ** -12), h(2.0 ** -12), sub),  # a hair more than half an ulp -> 1 + 2^-10: needs the exact sum (fp32 loses the 2^-24)
        (sub, sub, sub, sub),                         # subnormals: 2^-22
        (sub, h(6.1035e-05)),                         # subnormal + smallest normal
        (h(3.0), h(-3.0)),                            # cancels to +0
        (h(3.0), h(-1.0), h(-1.0), h(-1.0)),          # four terms cancel to +0
        (h(-0.0), h(-0.0), h(-0.0), h(-0.0)),         # -0
        (h(32768.0), sub),                            # 40 binades apart -> 2^15
        (h(40000.0), h(40000.0)),                     # leaves fp16 -> inf
        (h(-30000.0), h(-30000.0), h(-30000.0)),      # -> -inf
        (h(65504.0), h(15.0)),                        # 65519 < 65520: the largest finite value
        (h(65504.0), h(8.0), h(8.0)),                 # 65520: tie to the even mantissa = overflow -> inf
        (h(65504.0), h(65504.0), h(-65504.0), h(-65504.0)),  # passes 131008 on the way and comes back: exact sums do not overflow
    ]
    w = _one_group(vals)
    got, bad = fold(lib, w.view(np.uint16), 64)
    want = U.fold16(w)
    assert_same_bits(got, want.view(np.uint16))
    g = got.view(np.float16)[0, 0, 1, 1]
    assert g[0] == 2048.0 and g[1] == 2052.0 and g[2] == 1024.0 and g[3] == 1.0 and g[4] == h(1.0 + 2.0 ** -10) and g[5] == h(2.0 ** -22)
    assert got[0, 0, 1, 1, 7] == 0x0000 and got[0, 0, 1, 1, 8] == 0x0000 and got[0, 0, 1, 1, 9] == 0x8000   # +0, +0, -0 by their bits
    assert g[10] == 32768.0 and np.isposinf(g[11]) and np.isneginf(g[12]) and g[13] == 65504.0 and np.isposinf(g[14]) and g[15] == 0.0
    # every parity sees the group {1,2} x {1,2} split its own way; the count is over all of them
    assert bad == int((~np.isfinite(want)).sum()) and bad >= 3


def test_each_parity_sums_its_own_groups(lib):
    """distinct powers of two per tap: every folded weight names the taps it holds"""
    I = 64
    w = np.zeros((2, 3, 3, I), np.float16)
    for kh in range(3):
        for kw in range(3):
            w[:, kh, kw, :] = np.float16(2.0 ** (kh * 3 + kw))
    got, bad = fold(lib, w.view(np.uint16), I)
    assert bad == 0
    g = got.view(np.float16).astype(np.int64)
    rows = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    for q in range(4):
        for a in range(2):
            for b in range(2):
                want = sum(1 << (kh * 3 + kw) for kh in rows[q >> 1][a] for kw in rows[q & 1][b])
                assert (g[q, :, a, b, :] == want).all(), (q, a, b)


def test_a_wider_row_pitch_is_not_read(lib):
    r = np.random.default_rng(12)
    O, I, ldw = 5, 64, 9 * 64 + 72
    w = np.full((O, ldw), np.float16(7.0))     # what a wider pitch may hold: must not leak into the result
    w[:, :9 * I] = r.standard_normal((O, 9 * I)).astype(np.float16)
    got, bad = fold(lib, w.view(np.uint16), I, ldw)
    assert bad == 0
    assert_same_bits(got, U.fold16(w[:, :9 * I].reshape(O, 3, 3, I)).view(np.uint16))


def test_bad_arguments_are_refused(lib):
    w = np.zeros((1, 576), np.uint16)
    out = np.zeros((4, 1, 2, 2, 64), np.uint16)
    p, q = w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.tsd_debug_ups_fold_host(p, 1, 64, 575, q) < 0   # pitch narrower than the nine taps
    assert lib.tsd_debug_ups_fold_host(p, 0, 64, 576, q) < 0
    assert lib.tsd_debug_ups_fold_host(None, 1, 64, 576, q) < 0
    assert lib.tsd_debug_ups_fold_host(p, 1, 64, 576, None) < 0


# ---- the algebra, in float64 ---------------------------------------------------------------------------------------------------
def _conv3x3_of_upsampled(x, w):
    """x [B][Hs][Ws][C], w [O][3][3][C] -> [B][2 Hs][2 Ws][O]: nearest-2x upsample, zero pad 1, 3x3 convolution"""
    up = x.repeat(2, axis=1).repeat(2, axis=2)
    B, H, W, Cn = up.shape
    p = np.zeros((B, H + 2, W + 2, Cn))
    p[:, 1:-1, 1:-1] = up
    y = np.zeros((B, H, W, w.shape[0]))
    for kh in range(3):
        for kw in range(3):
            y += p[:, kh:kh + H, kw:kw + W] @ w[:, kh, kw, :].T
    return y


@pytest.mark.parametrize("B,Hs,Ws", [(1, 1, 1), (2, 3, 5), (3, 4, 2)])
def test_four_phase_convolutions_are_the_conv_of_the_upsampled_image(B, Hs, Ws):
    r = np.random.default_rng(100 + Hs)
    Cn, O = 7, 5
    x = r.standard_normal((B, Hs, Ws, Cn))
    w = r.standard_normal((O, 3, 3, Cn))
    ref = _conv3x3_of_upsampled(x, w)
    f = U.fold64(w)
    got = np.empty_like(ref)
    for q in range(4):
        got[:, (q >> 1)::2, (q & 1)::2] = U.gather2x2(x, q) @ f[q].reshape(O, 4 * Cn).T
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= 1e-12, err
    # ... and pixel by pixel, borders and corners included
    assert (np.abs(got - ref) <= 1e-12 * np.abs(ref).max()).all()
