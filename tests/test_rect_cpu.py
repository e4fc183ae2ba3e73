"""Rectangular latents without a GPU: the C ABI's new entries in the header, `tsd/_lib.py` and the Mojo shim, how a latent size is
parsed (an int or a pair), and `tsd.serve.SlotScheduler` against a recording stub session that is rectangular - and against one that
has only `L`, as the stubs of test_slots_cpu.py and test_slot_inpaint_cpu.py do."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tsd_diffusion_forward_hw", "tsd_decoder_forward_hw", "tsd_encoder_forward_hw", "tsd_latent_mask_hw_f32",
           "tsd_session_create_hw", "tsd_session_shape"]
STEPS, B, LH, LW = 3, 2, 2, 3
CTX = np.zeros((77, 768), dtype=np.float32)


def test_new_entries_are_declared_bound_exported_and_refuse_null(tsd_mod):
    from tsd._lib import TSD_E_ARG, ptr
    lib = tsd_mod._lib.lib()
    declared = tsd_mod._lib.declared_symbols()
    shim = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "mojo_shim", "tsd_ffi.mojo")).read()
    header = open(os.path.join(ROOT, "include", "tsd.h")).read()
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name          # bound with a signature, not only exported
        assert f'"{name}"' in shim and f"int {name}(" in header, name
    buf = np.zeros(4 * 8 * 16, dtype=np.float32)
    assert lib.tsd_diffusion_forward_hw(None, ptr(buf), ptr(buf), ptr(buf), 1, 8, 16, 77, ptr(buf)) == TSD_E_ARG
    assert lib.tsd_decoder_forward_hw(None, ptr(buf), 1, 8, 16, ptr(buf)) == TSD_E_ARG
    assert lib.tsd_encoder_forward_hw(None, ptr(buf), ptr(buf), 1, 64, 128, ptr(buf)) == TSD_E_ARG
    assert lib.tsd_latent_mask_hw_f32(None, ptr(buf), 1, 1, 2, 0, ptr(buf)) == TSD_E_ARG
    assert lib.tsd_session_create_hw(None, None, 1, 8, 16, 77, 0, None) == TSD_E_ARG
    assert lib.tsd_session_shape(None, None, None) == TSD_E_ARG
    # the shims that wrap the changed calls pass both sides
    for shim_file, call in (("vae_shim.mojo", "decoder_forward_hw"), ("vae_shim.mojo", "encoder_forward_hw"),
                            ("diffusion_shim.mojo", "diffusion_forward_hw")):
        text = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "mojo_shim", shim_file)).read()
        assert f"self.tsd.{call}(" in text and "x.dim1, x.dim2" in text, (shim_file, call)


def test_a_latent_size_is_an_int_or_a_pair(tsd_mod):
    from tsd._lib import latent_shape
    assert latent_shape(64) == (64, 64)
    assert latent_shape(np.int64(8)) == (8, 8)
    assert latent_shape((64, 96)) == (64, 96) and latent_shape([96, 64]) == (96, 64)
    assert latent_shape(np.array([8, 16])) == (8, 16)
    for bad in ((8,), (8, 16, 24), (8, 0), (-8, 16), (8.0, 16), (8, "16"), (True, 8), "8x16", None, 8.0, ()):
        with pytest.raises(ValueError):
            latent_shape(bad)


class RectStub:
    """The slot methods of `Session`, recording every call in order.  With `rect` the stub has `LH` / `LW` (and an `L` that is the
    pair the caller passed); without, only an int `L`."""

    def __init__(self, B, num_steps, LH, LW, rect=True):
        self.B, self.num_steps = B, num_steps
        if rect:
            self.L, self.LH, self.LW = (LH, LW), LH, LW
        else:
            assert LH == LW
            self.L = LH
        self.shape = (LH, LW)
        self.index, self.tag = [None] * B, [None] * B
        self.events = []

    def slot_start(self, b, context, uncond_context=None, latents=None, noise_at_start=False, seed=0, start_index=0, cfg_scale=7.5):
        assert 0 <= b < self.B and self.index[b] is None
        self.index[b], self.tag[b] = start_index, seed
        self.events.append(("start", b, seed, start_index))

    def slot_set_inpaint(self, b, mask, known=None):
        assert self.index[b] is not None
        self.events.append(("inpaint", b, np.array(mask, copy=True), np.array(known, copy=True)))

    def advance(self):
        active = [b for b in range(self.B) if self.index[b] is not None]
        assert active
        self.events.append(("advance", tuple(active)))
        done = []
        for b in active:
            self.index[b] += 1
            if self.index[b] == self.num_steps:
                self.index[b] = None
                done.append(b)
        self._last = {b: self.tag[b] for b in done}
        return done

    def slot_latents(self, b):
        return np.full((4,) + self.shape, self._last[b], dtype=np.float32)


def _lat(v, lh=LH, lw=LW):
    return np.full((4, lh, lw), float(v), dtype=np.float32)


def _block_mean(mask, mode="any", ctx=None):
    """stand-in for tsd.utils.latent_mask (the real one runs on the device): the 8x8 block mean, of a mask of any (B, 8h, 8w)"""
    m = np.asarray(mask, dtype=np.float32)
    b, h, w = m.shape
    return m.reshape(b, h // 8, 8, w // 8, 8).mean(axis=(2, 4)).astype(np.float32)


def test_the_scheduler_runs_a_rectangular_session_with_masks_of_both_layouts(tsd_mod, monkeypatch):
    """Latent masks (LH,LW) and (1,LH,LW) are used as given, pixel masks (8LH,8LW) and (1,8LH,8LW) go through tsd.utils.latent_mask;
    the mask that reaches slot_set_inpaint is (LH,LW) with the rows and columns where the request put them."""
    from tsd import utils
    from tsd.serve import Request, SlotScheduler, session_shape
    seen_px = []

    def fake(mask, mode="any", ctx=None):
        seen_px.append(np.shape(mask))
        return _block_mean(mask)

    monkeypatch.setattr(utils, "latent_mask", fake)
    stub = RectStub(B, STEPS, LH, LW)
    assert session_shape(stub) == (LH, LW)
    m_lat = np.arange(LH * LW, dtype=np.float32).reshape(LH, LW) / 8.0      # every cell its own value: a transposition shows
    px = np.zeros((8 * LH, 8 * LW), dtype=np.float32)
    px[:8, 16:] = 1.0          # latent cell (0, 2)
    px[8:, :8] = 0.5           # latent cell (1, 0)
    want_px = np.array([[0.0, 0.0, 1.0], [0.5, 0.0, 0.0]], dtype=np.float32)
    queue = [Request(0, CTX, CTX, 10),
             Request(1, CTX, CTX, 11, 7.5, _lat(1), 1.0, m_lat),
             Request(2, CTX, CTX, 12, 7.5, _lat(2), 1.0, m_lat[None]),
             Request(3, CTX, CTX, 13, 7.5, _lat(3), 1.0, px, "area"),
             Request(4, CTX, CTX, 14, 7.5, _lat(4), 1.0, px[None], "area")]
    got = dict(SlotScheduler(stub, iter(queue)))
    assert sorted(got) == [0, 1, 2, 3, 4] and all(got[k].shape == (4, LH, LW) for k in got)
    assert seen_px == [(1, 8 * LH, 8 * LW)] * 2
    masks = {}
    for n, e in enumerate(stub.events):
        if e[0] == "inpaint":
            prev = stub.events[n - 1]
            assert prev[0] == "start" and prev[1] == e[1]
            masks[prev[2]] = e[2]
    assert sorted(masks) == [11, 12, 13, 14]
    for seed, want in ((11, m_lat), (12, m_lat), (13, want_px), (14, want_px)):
        assert masks[seed].shape == (LH, LW) and masks[seed].dtype == np.float32 and np.array_equal(masks[seed], want), seed


@pytest.mark.parametrize("shape", [(LW, LH), (8 * LW, 8 * LH), (LH, LH), (8 * LH, 8 * LH), (2, LH, LW), (LH * LW,)])
def test_a_mask_of_the_transposed_or_a_square_shape_is_refused_by_a_rectangular_session(tsd_mod, shape):
    from tsd.serve import Request, SlotScheduler
    stub = RectStub(B, STEPS, LH, LW)
    with pytest.raises(ValueError):
        list(SlotScheduler(stub, iter([Request(0, CTX, CTX, 1, 7.5, _lat(1), 1.0, np.ones(shape, dtype=np.float32))])))
    assert stub.events == []


def test_the_scheduler_still_runs_a_session_that_has_only_L(tsd_mod, monkeypatch):
    from tsd import utils
    from tsd.serve import Request, SlotScheduler, session_shape
    monkeypatch.setattr(utils, "latent_mask", _block_mean)
    L = 2
    stub = RectStub(B, STEPS, L, L, rect=False)
    assert not hasattr(stub, "LH") and session_shape(stub) == (L, L)
    m = np.array([[0.0, 1.0], [0.25, 0.5]], dtype=np.float32)
    px = np.zeros((8 * L, 8 * L), dtype=np.float32)
    px[:8, 8:] = 1.0
    queue = [Request(0, CTX, CTX, 10), Request(1, CTX, CTX, 11, 7.5, _lat(1, L, L), 1.0, m),
             Request(2, CTX, CTX, 12, 7.5, _lat(2, L, L), 0.5, px[None], "area")]
    got = dict(SlotScheduler(stub, iter(queue)))
    assert sorted(got) == [0, 1, 2]
    inpaints = [e for e in stub.events if e[0] == "inpaint"]
    assert len(inpaints) == 2 and np.array_equal(inpaints[0][2], m)
    assert np.array_equal(inpaints[1][2], np.array([[0.0, 1.0], [0.0, 0.0]], dtype=np.float32))
    with pytest.raises(ValueError):
        list(SlotScheduler(RectStub(B, STEPS, L, L, rect=False),
                           iter([Request(0, CTX, CTX, 1, 7.5, _lat(1, L, L), 1.0, np.ones((L, L + 1), dtype=np.float32))])))
