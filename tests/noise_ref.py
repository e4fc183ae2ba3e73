"""Independent restatement of the seeded N(0,1) stream for the tests, in Python ints and the math module - no numpy integer arithmetic,
nothing imported from tsd.rng.  The stream is a pure function of (seed, stream id, element counter j):

    base = seed * 0x9E3779B97F4A7C15 + stream * 0xBF58476D1CE4E5B9       (mod 2^64)
    k1 = mix64(base + 2j) >> 40,  k2 = mix64(base + 2j + 1) >> 40          (24 bits each)
    z  = sqrt(-2 ln((k1 + 1) 2^-24)) * cos(pi k2 2^-23)                    float64, rounded to float32 once
"""
import math

import numpy as np

M64 = (1 << 64) - 1
NEW_ENTRIES = ("tsd_normal_fill_f32", "tsd_session_set_seeds", "tsd_session_seeds_active", "tsd_session_seed_latents",
               "tsd_session_add_noise_seeded", "tsd_session_set_inpaint_seeded")
STREAM_LATENTS, STREAM_ADD_NOISE, STREAM_STEP0 = 2, 4, 16
# (seed, stream, j) -> (k1, k2, float32 bits of z): from two independent implementations (numpy uint64 and Python ints)
KNOWN_ANSWERS = [
    (5, 78, 0, 16754296, 15463093, 0x3D3CC0DE),
    (5, 78, 1, 7549498, 16696099, 0x3FA1AFAD),
    (5, 78, 2, 15505225, 13213968, 0x3DBE6B11),
    (5, 78, 3, 15656456, 13253055, 0x3DBD2195),
    (M64, 16, (1 << 33) + 5, 13456822, 7175093, 0xBF18C288),
]


def mix64(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def keys(seed, stream, j):
    base = (seed * 0x9E3779B97F4A7C15 + stream * 0xBF58476D1CE4E5B9) & M64
    c = (base + 2 * j) & M64
    return mix64(c) >> 40, mix64((c + 1) & M64) >> 40


def normal_counter(seed, stream, n, offset=0):
    out = np.empty(n, dtype=np.float32)
    for e in range(n):
        k1, k2 = keys(seed, stream, offset + e)
        out[e] = math.sqrt(-2.0 * math.log((k1 + 1) * 2.0 ** -24)) * math.cos(math.pi * (k2 * 2.0 ** -23))
    return out


def moment_scores(z, z_next=None):
    """The scaled statistics the issue bounds by 5 (each is about |N(0,1)| for a true N(0,1) sample of this size) and the scaled
    Kolmogorov-Smirnov distance to Phi.  'lag1' and 'next_seed' are raw mean products, not centred and normalised correlations: for a
    stream whose mean is 0 and whose variance is 1 to within the bounds checked beside them the two differ by O(1/n)."""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    rn = math.sqrt(n)
    out = {
        "mean": abs(z.mean()) * rn,
        "var": abs(z.var() - 1.0) / math.sqrt(2.0 / n),
        "m3": abs((z ** 3).mean()) / math.sqrt(15.0 / n),
        "m4": abs((z ** 4).mean() - 3.0) / math.sqrt(96.0 / n),
        "lag1": abs(np.mean(z[:-1] * z[1:])) * rn,
    }
    if z_next is not None:
        out["next_seed"] = abs(np.mean(z * np.asarray(z_next, dtype=np.float64))) * rn
    s = np.sort(z) / math.sqrt(2.0)
    cdf = 0.5 * (1.0 + np.fromiter(map(math.erf, s.tolist()), dtype=np.float64, count=n))
    i = np.arange(1, n + 1)
    out["ks"] = max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n)) * rn
    return out
