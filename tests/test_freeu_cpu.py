"""CPU: FreeU's closed form against the literal FFT restatement of diffusers' fourier_filter, the table conventions against the oracle's
step table, the near misses of the model-level reference on the draw the GPU test uses, an fp32 emulation under the derived bound, and
the parts of the surface that need no device."""
import inspect
import os

import numpy as np
import pytest

import freeu_ref as F
from oracle.spec import FULL_UNET_STEPS
from util import TOL_MODEL, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ((2, 2), (2, 4), (4, 2), (4, 4), (6, 10), (8, 8), (12, 20), (16, 16), (3, 5), (64, 64))
SCALES = (0.9, 0.2, 1.0, -0.5)
NEW_SYMBOLS = ("tsd_model_set_freeu", "tsd_model_freeu", "tsd_freeu_f16")


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_closed_form_is_the_fft_restatement(plane):
    H, W = plane
    x = np.random.default_rng(H * 100 + W).normal(size=(3, 5, H, W))
    for s in SCALES:
        err = np.abs(F.fourier_filter_closed(x, s) - F.fourier_filter_fft(x, s)).max()
        assert err <= 1e-12, (plane, s, err)
    assert np.array_equal(F.fourier_filter_closed(x, 1.0), x)


def test_closed_form_on_the_special_planes():
    H, W = 8, 12
    y, x = np.arange(H)[:, None] * np.ones((1, W)), np.ones((H, 1)) * np.arange(W)[None, :]
    const = np.full((H, W), 0.75)
    cosy = np.cos(2 * np.pi * y / H)
    checker = np.where((y + x) % 2 == 0, 1.0, -1.0)
    for s in SCALES:
        assert np.abs(F.fourier_filter_closed(const, s) - s * const).max() <= 1e-12
        # a cosine along y has half its energy in bin fy = -1 and half in fy = +1, and the mask holds only the first: (1 + s) / 2, not s
        assert np.abs(F.fourier_filter_closed(cosy, s) - 0.5 * (1.0 + s) * cosy).max() <= 1e-12
        assert np.abs(F.fourier_filter_closed(checker, s) - checker).max() <= 1e-12      # P = 0: all its energy sits at Nyquist
        assert np.abs(F.fourier_filter_fft(cosy, s) - 0.5 * (1.0 + s) * cosy).max() <= 1e-12
        two = np.array([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])           # H = 2: bin -1 is the Nyquist bin, the whole cosine: s
        assert np.abs(F.fourier_filter_fft(two, s) - s * two).max() <= 1e-12 and np.abs(F.fourier_filter_closed(two, s) - s * two).max() <= 1e-12


def test_hidden_modes():
    g = np.random.default_rng(3)
    h = g.normal(size=(2, 4, 6, 16))
    c = F.hidden_constant(h, 1.5)
    assert np.array_equal(c[..., 8:], h[..., 8:]) and np.allclose(c[..., :8], 1.5 * h[..., :8])
    m = F.hidden_modulated(h, 1.5)
    n = F.modulation(h)
    assert n.min() == 0.0 and n.max() == 1.0 and np.array_equal(m[..., 8:], h[..., 8:])
    assert np.allclose(m[..., :8], (0.5 * n + 1.0) * h[..., :8])
    flat = np.broadcast_to(h[:, :1, :1, :], h.shape)          # every pixel the same vector: hi == lo, n = 0
    assert np.array_equal(F.hidden_modulated(flat, 1.5), flat)


def test_table_conventions_follow_the_widths_of_the_step_table():
    import tsd
    widths = F.hidden_widths()
    assert widths == list(tsd.free_u.FREEU_HIDDEN_WIDTHS) and len(widths) == tsd.free_u.FREEU_BLOCKS == 12
    assert len(F.POP_LAYERS) == 12 and all(FULL_UNET_STEPS[i - 1][2] == "pop" for i in F.POP_LAYERS)
    b, s = tsd.freeu_table(1.5, 1.6, 0.9, 0.2)
    assert b.dtype == s.dtype == np.float32
    assert b.tolist() == [np.float32(v) for v in [1.5] * 3 + [1.6] * 3 + [1.0] * 6]
    assert s.tolist() == [np.float32(v) for v in [0.9] * 3 + [0.2] * 3 + [1.0] * 6]
    b, s = tsd.freeu_table(1.5, 1.6, 0.9, 0.2, convention="channels")
    for j, c in enumerate(widths):
        want = {1280: (1.5, 0.9), 640: (1.6, 0.2), 320: (1.0, 1.0)}[c]
        assert (b[j], s[j]) == (np.float32(want[0]), np.float32(want[1])), j
    with pytest.raises(ValueError):
        tsd.freeu_table(1.5, 1.6, 0.9, 0.2, convention="comfy")


def test_surface_without_a_device():
    import tsd
    from tsd.free_u import freeu_arguments, freeu_scope
    declared = tsd._lib.declared_symbols()
    header = open(os.path.join(ROOT, "include", "tsd.h")).read()
    shim = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "mojo_shim", "tsd_ffi.mojo")).read()
    lib = tsd._lib.lib()
    for name in NEW_SYMBOLS + ("tsd_debug_freeu_run",):
        assert name in declared and hasattr(lib, name) and name in header
    for name in NEW_SYMBOLS:
        assert f'"{name}"' in shim
    for const in ("TSD_FREEU_BLOCKS: Int32 = 12", "TSD_FREEU_CONSTANT: Int32 = 0", "TSD_FREEU_MODULATED: Int32 = 1"):
        assert const in shim
    assert "#define TSD_FREEU_BLOCKS 12" in header and "TSD_FREEU_CONSTANT = 0, TSD_FREEU_MODULATED = 1" in header
    for fn in (tsd.generate, tsd.generate_stream):
        assert inspect.signature(fn).parameters["freeu"].default is None
    for name in ("set_freeu", "clear_freeu", "freeu"):
        assert hasattr(tsd.Diffusion, name)
    b, s, mode = freeu_arguments(1.5, 1.6, 0.9, 0.2, modulated=True)
    assert mode == tsd.free_u.FREEU_MODULATED and b[0] == 1.5 and s[3] == np.float32(0.2)
    b, s, mode = freeu_arguments(table=(np.arange(12), np.ones(12)))
    assert mode == tsd.free_u.FREEU_CONSTANT and b.dtype == np.float32 and b[11] == 11
    with pytest.raises(ValueError):
        freeu_arguments(1.5, 1.6, 0.9)                                   # s2 missing
    with pytest.raises(ValueError):
        freeu_arguments(1.5, 1.6, 0.9, 0.2, table=(np.ones(12), np.ones(12)))
    with pytest.raises(ValueError):
        freeu_arguments(table=(np.ones(11), np.ones(12)))
    with pytest.raises(ValueError):
        with freeu_scope(None, [1.5, 1.6, 0.9, 0.2]):                    # not a dict
            pass
    with freeu_scope(None, None):                                        # None: the model is not touched
        pass
    # the C entries refuse a NULL model before anything else (no device needed)
    assert lib.tsd_model_set_freeu(None, None, None, 0) == tsd._lib.TSD_E_ARG
    assert lib.tsd_model_freeu(None, None, None, None) == tsd._lib.TSD_E_ARG


def _emulate_skip_fp32(r, s):
    """The launch's arithmetic in numpy fp32 (tables rounded once, fp32 sums in numpy's own order, one rounding to fp16)."""
    B, H, W, C = r.shape
    f = np.float32
    y, x = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    cy, sy = np.cos(2 * np.pi * y / H).astype(f)[:, None], np.sin(2 * np.pi * y / H).astype(f)[:, None]
    cx, sx = np.cos(2 * np.pi * x / W).astype(f)[None, :], np.sin(2 * np.pi * x / W).astype(f)[None, :]
    one = np.ones((H, W), f)
    basis = [one, cy * one, sy * one, cx * one, sx * one, cy * cx - sy * sx, sy * cx + cy * sx]
    r32 = np.moveaxis(r.astype(f), -1, 1)
    N = np.zeros_like(r32)
    for c in basis:
        N += (r32 * c).sum((-2, -1), keepdims=True, dtype=f) * c
    out = r32 + f((s - 1.0) / (H * W)) * N
    return np.moveaxis(out, 1, -1).astype(np.float16)


@pytest.mark.parametrize("shape", ((2, 2, 2, 8), (1, 6, 10, 16), (1, 64, 64, 8)), ids=str)
def test_an_fp32_emulation_lies_under_the_derived_bound(shape):
    g = np.random.default_rng(5)
    r = g.normal(size=shape).astype(np.float16)
    h = (g.normal(size=shape) + np.linspace(0, 1, shape[1] * shape[2]).reshape(1, shape[1], shape[2], 1)).astype(np.float16)
    worst = 0.0
    for s in (0.9, 0.2, -0.5):
        y, bound = F.skip_bound(r, s)
        ratio = np.abs(_emulate_skip_fp32(r, s).astype(np.float64) - y) / bound
        assert ratio.max() <= 1.0, (shape, s, ratio.max())
        worst = max(worst, ratio.max())
    assert worst > 0.2          # the bound is not idle: the fp16 rounding alone comes close to it
    for b in (1.5, 0.5):
        y, bound = F.hidden_bound(h, b, F.CONSTANT)
        got = h.astype(np.float32).copy()
        got[..., : shape[3] // 2] *= np.float32(b)
        assert (np.abs(got.astype(np.float16).astype(np.float64) - y) <= bound).all()
        y, bound = F.hidden_bound(h, b, F.MODULATED)
        h32 = h.astype(np.float32)
        m = h32.sum(-1, keepdims=True, dtype=np.float32) / np.float32(shape[3])
        lo, hi = m.min((1, 2), keepdims=True), m.max((1, 2), keepdims=True)
        n = (m - lo) / (hi - lo)
        got = h32.copy()
        got[..., : shape[3] // 2] *= np.float32(b - 1.0) * n + np.float32(1.0)
        assert (np.abs(got.astype(np.float16).astype(np.float64) - y) <= bound).all()
        assert (bound[..., shape[3] // 2:] == 0).all()


def test_near_misses_are_far_from_the_reference_on_the_shared_draw():
    """Kind 6 at 16 x 16, every (convention, mode): FreeU moves the forward by more than 10 TOL_MODEL, and so does each way of getting it
    wrong - the scaled half being the upper channels, the filter on the hidden tensor, s applied as s - 1, the other convention."""
    import tsd
    from controlnet_ref import draw_params
    kind = "diffusion_sd15_torch"
    P = draw_params(tsd.param_specs(kind), F.MODEL_SEED)
    lat, ctx, temb = F.model_inputs(kind, 16, 16)
    plain = F.diffusion_freeu(P, lat[0], ctx[0], temb[0], None, tn=True)
    assert rel_l2(plain, __import__("controlnet_ref").diffusion_sd15_controlled(P, lat[0], ctx[0], temb[0], None, 0.0, tn=True)) == 0.0
    for conv, other in (("diffusers", "channels"), ("channels", "diffusers")):
        for mode in (F.CONSTANT, F.MODULATED):
            tab = tsd.freeu_table(convention=conv, **F.MODEL_VALUES)
            ref = F.diffusion_freeu(P, lat[0], ctx[0], temb[0], tab, mode, tn=True)
            far = {"plain": rel_l2(ref, plain),
                   "swapped": rel_l2(F.diffusion_freeu(P, lat[0], ctx[0], temb[0], tsd.freeu_table(convention=other, **F.MODEL_VALUES), mode, tn=True), ref)}
            for miss in F.NEAR_MISSES:
                far[miss] = rel_l2(F.diffusion_freeu(P, lat[0], ctx[0], temb[0], tab, mode, tn=True, miss=miss), ref)
            print(f"[freeu] {conv} mode {mode}: " + " ".join(f"{k} {v:.3f}" for k, v in far.items()))
            assert min(far.values()) > 10 * TOL_MODEL, (conv, mode, far)
