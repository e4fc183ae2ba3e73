"""fp64 reference of guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", eq. 15-16), as
include/tsd.h states it.  Per sample, with c the conditional and u the unconditional eps of n elements, s the guidance scale, phi in [0, 1]:

    e_i   = (c_i - u_i) * s + u_i                 formed step by step in float32: the update kernel's own combine
    var_c = sum c^2 / n - (sum c / n)^2           float64 sums of the float32 values (a product of two float32 values is exact there)
    var_e likewise over e
    g     = phi * sqrt(var_c / var_e) + (1 - phi)
    c'    = float32(g) * c,  u' = float32(g) * u

g = 1 exactly when var_e is not finite, var_e <= 0 or var_c is not finite; a var_c below zero counts as zero.

`kappa` is the conditioning of the one-pass variance: max over x in {c, e} of sum x^2 / (n var_x).  A relative error d in the sums moves the
variance by up to d * kappa, relatively - which is how far the ORDER of a float64 summation can move g (d <= n 2^-53 for any order).
"""
import numpy as np


def combine_f32(c, u, s):
    """e = (c - u) * s + u with one float32 rounding per operation."""
    c, u = np.asarray(c, dtype=np.float32), np.asarray(u, dtype=np.float32)
    d = (c - u).astype(np.float32)
    ds = (d * np.float32(s)).astype(np.float32)
    return (ds + u).astype(np.float32)


def moments(x):
    """(sum x^2 / n, var) of a float32 tensor in float64, one pass."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64).ravel()
    n = x.size
    with np.errstate(all="ignore"):
        m2 = float((x * x).sum()) / n
        m1 = float(x.sum()) / n
        return m2, m2 - m1 * m1


def rescale_factor(c, u, s, phi):
    """-> (g float64, kappa) of ONE sample."""
    e = combine_f32(c, u, s)
    c2, var_c = moments(c)
    e2, var_e = moments(e)
    if not (np.isfinite(var_e) and var_e > 0.0 and np.isfinite(var_c)):
        return 1.0, float("inf")
    kappa = max(c2 / var_c if var_c > 0.0 else float("inf"), e2 / var_e)
    phi = float(np.float32(phi))
    g = phi * np.sqrt(max(var_c, 0.0) / var_e) + (1.0 - phi)
    return float(g), float(kappa)


def rescale(c, u, s, phi):
    """Batch (B, ...): s and phi scalars or (B,) -> (c', u', g float32 (B,), g float64 (B,), kappa (B,)).  A sample with phi = 0 is its
    input, bit for bit, with g = 1."""
    c, u = np.asarray(c, dtype=np.float32), np.asarray(u, dtype=np.float32)
    B = c.shape[0]
    s = np.broadcast_to(np.asarray(s, dtype=np.float32), (B,))
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float32), (B,))
    co, uo = c.copy(), u.copy()
    g32, g64, kap = np.ones(B, dtype=np.float32), np.ones(B), np.zeros(B)
    for b in range(B):
        if phi[b] == 0:
            continue
        g64[b], kap[b] = rescale_factor(c[b], u[b], s[b], phi[b])
        g32[b] = np.float32(g64[b])
        with np.errstate(all="ignore"):
            co[b] = (g32[b] * c[b]).astype(np.float32)
            uo[b] = (g32[b] * u[b]).astype(np.float32)
    return co, uo, g32, g64, kap


def ulps_f32(a, b):
    """Distance of two positive finite float32 values in units in the last place."""
    ia = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
