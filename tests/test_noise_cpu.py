"""Seeded device-side noise, the part that needs no GPU: the host twin `tsd.rng.normal_counter` gives the known answers bitwise, is a
pure function of the counter, agrees with an independent Python-int restatement and has the moments of N(0,1); the new entries are
declared, exported and bound, refuse NULL handles before any device work, and `generate` refuses two sources of noise."""
import ctypes as C
import os

import numpy as np
import pytest

import noise_ref
from noise_ref import KNOWN_ANSWERS, M64, NEW_ENTRIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 2, 12345, (1 << 63) + 7, M64]
STREAMS = [2, 3, 4]
N = 1 << 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. known answers -----------------------------------------------------------------------------------------------------------------
def test_the_twin_gives_the_known_answers_bitwise(tsd_mod):
    for seed, stream, j, k1, k2, bits in KNOWN_ANSWERS:
        assert noise_ref.keys(seed, stream, j) == (k1, k2), (seed, stream, j)
        z = tsd_mod.rng.normal_counter(seed, stream, 1, offset=j)
        assert z.dtype == np.float32 and z.shape == (1,)
        assert int(_bits(z)[0]) == bits, (seed, stream, j, hex(int(_bits(z)[0])), hex(bits))
    z = tsd_mod.rng.normal_counter(5, 78, 4)
    assert [int(b) for b in _bits(z)] == [a[5] for a in KNOWN_ANSWERS[:4]]


# ---- 2. counter purity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,stream", [(0, 2), (12345, 16), (M64, 4), ((1 << 63) + 7, 65)])
def test_the_twin_is_a_pure_function_of_the_counter_and_equals_the_restatement(tsd_mod, seed, stream):
    rng = tsd_mod.rng
    whole = rng.normal_counter(seed, stream, 1000)
    part = rng.normal_counter(seed, stream, 200, offset=300)
    assert np.array_equal(_bits(part), _bits(whole[300:500]))
    assert np.array_equal(_bits(part), _bits(noise_ref.normal_counter(seed, stream, 200, offset=300)))
    far = (1 << 33) + 5
    assert np.array_equal(_bits(rng.normal_counter(seed, stream, 50, offset=far)), _bits(noise_ref.normal_counter(seed, stream, 50, offset=far)))
    # |z| <= sqrt(48 ln 2), and `normal` (the Box-Muller of the other host streams) is left alone: another stream altogether
    assert np.abs(whole).max() <= 5.78 and not np.array_equal(whole, rng.normal(seed & 0xFFFFFFFF, stream, 1000))


# ---- 3. moments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("seed", SEEDS, ids=lambda s: hex(s))
def test_moments_of_the_twin(tsd_mod, seed, stream):
    """n = 2^20 values: each scaled statistic is about |N(0,1)| for a true normal sample, bound 5 (about 6e-7 per statistic); the scaled
    Kolmogorov-Smirnov distance to Phi is at most 1.36 on exactly these inputs."""
    z = tsd_mod.rng.normal_counter(seed, stream, N)
    z_next = tsd_mod.rng.normal_counter((seed + 1) & M64, stream, N)
    sc = noise_ref.moment_scores(z, z_next)
    print(f"[noise] twin seed={seed:#x} stream={stream}: " + " ".join(f"{k}={v:.2f}" for k, v in sc.items()))
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.78
    for k in ("mean", "var", "m3", "m4", "lag1", "next_seed"):
        assert sc[k] <= 5.0, (k, sc[k])
    assert sc["ks"] <= 1.36, sc["ks"]


# ---- 4. the C ABI and the Python surface ----------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound(tsd_mod):
    lib = tsd_mod._lib.lib()
    declared = tsd_mod._lib.declared_symbols()
    nargs = {"tsd_normal_fill_f32": 6, "tsd_session_set_seeds": 2, "tsd_session_seeds_active": 1, "tsd_session_seed_latents": 1,
             "tsd_session_add_noise_seeded": 2, "tsd_session_set_inpaint_seeded": 3}
    assert set(nargs) == set(NEW_ENTRIES)
    for name in NEW_ENTRIES:
        assert name in declared, name
        fn = getattr(lib, name)          # AttributeError: not exported
        assert fn.argtypes is not None and len(fn.argtypes) == nargs[name] and fn.restype is C.c_int, name
    assert callable(tsd_mod.normal_fill) and callable(tsd_mod.rng.normal_counter)
    for name in ("set_seeds", "seed_latents", "add_noise_seeded"):
        assert callable(getattr(tsd_mod.Session, name)), name
    assert isinstance(tsd_mod.Session.seeds_active, property)
    import inspect
    assert "seeded" in inspect.signature(tsd_mod.Session.set_inpaint).parameters
    assert inspect.signature(tsd_mod.generate).parameters["seeds"].default is None
    shim = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "mojo_shim", "tsd_ffi.mojo")).read()
    for name in NEW_ENTRIES:
        assert '"%s"' % name in shim, name


def test_entries_refuse_null_handles_without_a_device(tsd_mod):
    from tsd._lib import TSD_E_ARG, TSD_E_SHAPE, ptr
    lib = tsd_mod._lib.lib()
    out = np.zeros(4, dtype=np.float32)
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)   # a context that is no context: only validation returns from it
    assert lib.tsd_normal_fill_f32(None, 1, 2, 0, 4, ptr(out)) == TSD_E_ARG
    assert lib.tsd_normal_fill_f32(fake, 1, 2, 0, 4, None) == TSD_E_ARG
    assert lib.tsd_normal_fill_f32(fake, 1, 2, 0, 0, ptr(out)) == TSD_E_SHAPE
    assert lib.tsd_normal_fill_f32(fake, 1, 2, 0, -3, ptr(out)) == TSD_E_SHAPE
    seeds = (C.c_uint64 * 2)(1, 2)
    assert lib.tsd_session_set_seeds(None, seeds) == TSD_E_ARG
    assert lib.tsd_session_seeds_active(None) == TSD_E_ARG
    assert lib.tsd_session_seed_latents(None) == TSD_E_ARG
    assert lib.tsd_session_add_noise_seeded(None, 0) == TSD_E_ARG
    assert lib.tsd_session_set_inpaint_seeded(None, ptr(out), ptr(out)) == TSD_E_ARG


def test_generate_refuses_two_sources_of_noise(tsd_mod):
    """seeds with noise, or seeds with latents: ValueError before any session or device work (the models are never touched)."""
    ctx = np.zeros((2, 77, 768), dtype=np.float32)
    with pytest.raises(ValueError):
        tsd_mod.generate(None, None, ctx, seeds=[1, 2], noise=np.zeros((2, 2, 4, 8, 8), dtype=np.float32), L=8, inference_steps=2)
    with pytest.raises(ValueError):
        tsd_mod.generate(None, None, ctx, seeds=[1, 2], latents=np.zeros((2, 4, 8, 8), dtype=np.float32), L=8, inference_steps=2)
