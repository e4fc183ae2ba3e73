"""Masked denoising, the part that needs no GPU: the new entries are declared, exported and bound, their enum is pinned, they refuse
bad arguments before any device work, `generate` validates its mask arguments before it creates a session, and the rounding count the
GPU test bounds the blend kernel with holds for the kernel's sequence of operations restated in numpy float32."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from inpaint_ref import MASK_ANY, MASK_AREA, NEW_ENTRIES, U, blend_f64, known_f32, latent_mask_np, mask_per_element
from util import randn, uni

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entries_are_declared_exported_and_bound(tsd_mod):
    lib = tsd_mod._lib.lib()
    declared = tsd_mod._lib.declared_symbols()
    nargs = {"tsd_latent_mask_f32": 6, "tsd_inpaint_blend_f32": 10, "tsd_session_set_inpaint": 4, "tsd_session_inpaint_active": 1}
    for name in NEW_ENTRIES:
        assert name in declared, name
        fn = getattr(lib, name)          # AttributeError: not exported
        assert fn.argtypes is not None and len(fn.argtypes) == nargs[name] and fn.restype is C.c_int, name
    for name in ("latent_mask", "inpaint_blend"):
        assert callable(getattr(tsd_mod, name))
    assert hasattr(tsd_mod.Session, "set_inpaint") and isinstance(tsd_mod.Session.inpaint_active, property)


def test_mask_mode_values_are_pinned(tsd_mod):
    hdr = open(os.path.join(ROOT, "include", "tsd.h")).read()
    m = re.search(r"typedef enum tsd_mask_mode \{([^}]*)\} tsd_mask_mode;", hdr)
    assert m and [p.strip() for p in m.group(1).split(",")] == ["TSD_MASK_AREA = 0", "TSD_MASK_ANY = 1"]
    assert tsd_mod._lib.MASK_MODES == {"area": 0, "any": 1} and (MASK_AREA, MASK_ANY) == (0, 1)
    assert tsd_mod._lib.mask_mode("ANY") == 1 and tsd_mod._lib.mask_mode("area") == 0 and tsd_mod._lib.mask_mode("most") == -1


def test_entries_refuse_bad_arguments_without_a_device(tsd_mod):
    """NULL handles, a bad enum, bad shapes and out-of-range mask values are refused before the context is touched: the calls below
    pass a context that is no context (zeroed memory), which only a call that validates first returns from with these codes."""
    from tsd._lib import TSD_E_ARG, TSD_E_SHAPE, ptr
    lib = tsd_mod._lib.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    B, L = 1, 1
    px, lat = np.zeros((B, 8, 8), np.float32), np.zeros((B, L, L), np.float32)
    assert lib.tsd_latent_mask_f32(None, ptr(px), B, L, 1, ptr(lat)) == TSD_E_ARG
    assert lib.tsd_latent_mask_f32(ctx, None, B, L, 1, ptr(lat)) == TSD_E_ARG
    assert lib.tsd_latent_mask_f32(ctx, ptr(px), B, L, 1, None) == TSD_E_ARG
    for mode in (2, -1):
        assert lib.tsd_latent_mask_f32(ctx, ptr(px), B, L, mode, ptr(lat)) == TSD_E_ARG
        assert "mode" in tsd_mod._lib.last_error()
    for b, l in ((0, 1), (1, 0), (1, -8)):
        assert lib.tsd_latent_mask_f32(ctx, ptr(px), b, l, 0, ptr(lat)) == TSD_E_SHAPE
    for bad in (1.5, -0.001, np.nan, np.inf):
        p = px.copy()
        p[0, 7, 7] = bad
        assert lib.tsd_latent_mask_f32(ctx, ptr(p), B, L, 0, ptr(lat)) == TSD_E_ARG, bad

    x, m = np.zeros((1, 4, 3), np.float32), np.ones((1, 3), np.float32)
    assert lib.tsd_inpaint_blend_f32(None, ptr(x), ptr(m), ptr(x), None, 1, 3, 1.0, 0.0, ptr(x)) == TSD_E_ARG
    for args in ((None, ptr(m), ptr(x), ptr(x)), (ptr(x), None, ptr(x), ptr(x)), (ptr(x), ptr(m), None, ptr(x)), (ptr(x), ptr(m), ptr(x), None)):
        assert lib.tsd_inpaint_blend_f32(ctx, args[0], args[1], args[2], None, 1, 3, 1.0, 0.0, args[3]) == TSD_E_ARG
    for b, hw in ((0, 3), (1, 0), (-1, 3)):
        assert lib.tsd_inpaint_blend_f32(ctx, ptr(x), ptr(m), ptr(x), None, b, hw, 1.0, 0.0, ptr(x)) == TSD_E_SHAPE

    assert lib.tsd_session_set_inpaint(None, ptr(m), ptr(x), None) == TSD_E_ARG
    assert lib.tsd_session_set_inpaint(None, None, None, None) == TSD_E_ARG
    assert lib.tsd_session_inpaint_active(None) < 0


def test_generate_validates_the_mask_before_it_creates_a_session(tsd_mod, monkeypatch):
    import tsd.pipeline as pipeline

    def no_session(*a, **k):
        raise AssertionError("generate() created a session before it validated its arguments")

    monkeypatch.setattr(pipeline, "Session", no_session)
    monkeypatch.setattr(pipeline, "latent_mask", no_session)
    L = 8
    ctx = np.zeros((1, 77, 768), np.float32)
    mask, image = np.ones((1, 1, 8 * L, 8 * L), np.float32), np.zeros((1, 3, 8 * L, 8 * L), np.float32)
    with pytest.raises(ValueError, match="input_image"):
        pipeline.generate(None, None, ctx, L=L, mask=mask)
    with pytest.raises(ValueError, match="input_image"):
        pipeline.generate(None, None, ctx, L=L, mask=mask, input_image=image)          # no encoder
    with pytest.raises(ValueError, match="input_image"):
        pipeline.generate(None, None, ctx, L=L, mask=mask, encoder=object())           # no image
    for bad in (mask[:, :, :32], mask[0, 0], np.ones((2, 1, 8 * L, 8 * L), np.float32), np.ones((1, 3, 8 * L, 8 * L), np.float32)):
        with pytest.raises(ValueError, match="mask must have shape"):
            pipeline.generate(None, None, ctx, L=L, mask=bad, input_image=image, encoder=object())


def _kernel_order_f32(x, mask, known, noise, a_prev, s_prev):
    """k_inpaint_blend's sequence of operations in numpy float32 (one rounding each, no fma)."""
    a, s = np.float32(a_prev), np.float32(s_prev)
    m = mask_per_element(mask, x.shape).astype(np.float32)
    k = a * known
    if noise is not None:
        k = k + s * noise
    om = np.float32(1.0) - m
    out = m * x + om * k
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("with_noise", [True, False])
def test_the_blend_formula_holds_its_rounding_count_and_has_exact_ends(with_noise):
    """The bound the GPU test asserts, k = 5 roundings through the worst term, on the same sequence of fp32 operations in numpy; and the
    exact ends of m x + (1 - m) k that k + m (x - k) does not have."""
    B, hw = 3, 5839
    x, known, z = (randn(1110 + k, B, 4, hw).astype(np.float32) for k in range(3))
    noise = z if with_noise else None
    soft = (uni(1113, 0.5, B * hw) + 0.5).astype(np.float32)
    cls = (np.arange(B * hw) * 7 + 3) % 3
    mask = np.where(cls == 0, np.float32(0), np.where(cls == 1, np.float32(1), soft)).astype(np.float32).reshape(B, hw)
    a_prev, s_prev = np.float32(0.8131), np.float32(0.5821)
    got = _kernel_order_f32(x, mask, known, noise, a_prev, s_prev)
    ref, terms = blend_f64(x, mask, known, noise, a_prev, s_prev)
    assert (np.abs(got.astype(np.float64) - ref) <= 5 * U * terms).all()
    M = mask_per_element(mask, x.shape)
    k32 = known_f32(known, noise, a_prev, s_prev)
    assert np.array_equal(got[M == 1].view(np.uint32), x[M == 1].view(np.uint32))
    assert np.array_equal(got[M == 0].view(np.uint32), k32[M == 0].view(np.uint32))
    other = k32 + M.astype(np.float32) * (x - k32)        # the form the kernel does not use
    assert not np.array_equal(other[M == 1], x[M == 1])


def test_latent_mask_restatement():
    m = np.zeros((1, 16, 16), np.float32)
    m[0, 0, 0], m[0, 9, 12] = 1.0, 0.5
    assert np.array_equal(latent_mask_np(m, MASK_ANY), np.array([[[1, 0], [0, 1]]], np.float32))
    assert np.array_equal(latent_mask_np(m, MASK_AREA), np.array([[[1 / 64, 0], [0, 0.5 / 64]]]))
    binary = (uni(1130, 1.0, 2, 64, 64) > 0.9).astype(np.float32)
    assert 0 < (latent_mask_np(binary, MASK_ANY) == 0).sum() < 128    # the GPU test's binary mask has empty and non-empty blocks
