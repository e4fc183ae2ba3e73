"""Inpainting in slot sessions without a GPU: the C ABI's new symbols, `tsd.serve.Request`'s mask fields and `tsd.serve.SlotScheduler`
against a recording fake session, and the text of advance() (no copy from the host)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, B, L = 4, 2, 2
SYMBOLS = ["tsd_session_slot_set_inpaint", "tsd_session_slot_inpaint_active"]


def test_symbols_are_declared_exported_and_refuse_null(tsd_mod):
    from tsd._lib import TSD_E_ARG, ptr
    lib = tsd_mod._lib.lib()
    declared = tsd_mod._lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    buf = np.zeros(4 * 8 * 8, dtype=np.float32)
    assert lib.tsd_session_slot_set_inpaint(None, 0, ptr(buf), ptr(buf)) == TSD_E_ARG
    assert lib.tsd_session_slot_inpaint_active(None, 0) == TSD_E_ARG
    for name in ("slot_set_inpaint", "slot_inpaint_active"):
        assert callable(getattr(tsd_mod.Session, name)), name
    shim = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "mojo_shim", "tsd_ffi.mojo")).read()
    header = open(os.path.join(ROOT, "include", "tsd.h")).read()
    for name in SYMBOLS:
        assert f'"{name}"' in shim and f"int {name}(" in header, name
    assert "Inpainting in slots is out of scope" not in header


class FakeSession:
    """The slot methods of `Session`, recording every call in order; a finished slot's latents are its request's seed."""

    def __init__(self, B, num_steps, L):
        self.B, self.num_steps, self.L = B, num_steps, L
        self.index, self.tag = [None] * B, [None] * B
        self.events = []   # ("start", b, seed, start_index) / ("inpaint", b, mask, known) / ("advance", active slots)

    def slot_start(self, b, context, uncond_context=None, latents=None, noise_at_start=False, seed=0, start_index=0, cfg_scale=7.5):
        assert 0 <= b < self.B and self.index[b] is None and noise_at_start == (latents is not None)
        self.index[b], self.tag[b] = start_index, seed
        self.events.append(("start", b, seed, start_index))

    def slot_set_inpaint(self, b, mask, known=None):
        assert self.index[b] is not None, "slot_set_inpaint on a slot that is not active"
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
        return np.full((4, self.L, self.L), self._last[b], dtype=np.float32)


CTX = np.zeros((77, 768), dtype=np.float32)


def _lat(v):
    return np.full((4, L, L), float(v), dtype=np.float32)


def test_request_keeps_its_seven_positional_fields_and_gains_two_trailing_ones(tsd_mod):
    from tsd.serve import Request
    assert Request._fields == ("id", "context", "uncond", "seed", "cfg_scale", "latents", "strength", "mask", "mask_mode")
    r = Request("a", CTX, CTX, 5, 3.0, _lat(1), 0.5)          # the seven-field positional form
    assert (r.seed, r.cfg_scale, r.strength, r.mask, r.mask_mode) == (5, 3.0, 0.5, None, "any")
    r = Request("b", CTX)
    assert (r.uncond, r.seed, r.cfg_scale, r.latents, r.strength, r.mask, r.mask_mode) == (None, 0, 7.5, None, None, None, "any")
    m = np.ones((L, L), dtype=np.float32)
    assert Request("c", CTX, CTX, 1, 7.5, _lat(2), 1.0, m, "area").mask_mode == "area"


def test_the_scheduler_sets_inpainting_right_after_slot_start_for_mask_requests_only(tsd_mod, monkeypatch):
    """Requests 0 (txt2img), 1 (latent mask (L,L)), 2 (img2img), 3 (pixel mask (1,8L,8L), "area"), 4 (latent mask (1,L,L)), 5 (a seven-field
    tuple): slot_set_inpaint follows the request's own slot_start at once - same slot, the request's latents as `known`, before the next
    advance - and nothing else calls it.  A pixel mask goes through tsd.utils.latent_mask with the request's mode (stubbed here: the real
    one runs on the device)."""
    from tsd import utils
    from tsd.serve import Request, SlotScheduler
    calls = []

    def fake_latent_mask(mask, mode="any", ctx=None):
        m = np.asarray(mask, dtype=np.float32)
        assert m.shape == (1, 8 * L, 8 * L)
        calls.append(mode)
        return m.reshape(1, L, 8, L, 8).mean(axis=(2, 4)).astype(np.float32)

    monkeypatch.setattr(utils, "latent_mask", fake_latent_mask)
    m1 = np.array([[0.0, 1.0], [0.25, 0.5]], dtype=np.float32)
    m4 = np.array([[1.0, 0.0], [0.75, 0.0]], dtype=np.float32)
    px = np.zeros((8 * L, 8 * L), dtype=np.float32)
    px[:8, 8:] = 1.0
    px[8:, :8] = 0.5
    queue = [Request(0, CTX, CTX, 10),
             Request(1, CTX, CTX, 11, 7.5, _lat(1), 1.0, m1),
             Request(2, CTX, CTX, 12, 7.5, _lat(2), 0.5),
             Request(3, CTX, CTX, 13, 7.5, _lat(3), 0.5, mask=px[None], mask_mode="area"),
             Request(4, CTX, CTX, 14, 7.5, _lat(4), 0.75, m4[None]),
             (5, CTX, CTX, 15, 7.5, _lat(5), 0.25)]
    fake = FakeSession(B, STEPS, L)
    got = dict(SlotScheduler(fake, iter(queue)))
    assert sorted(got) == list(range(6)) and all(float(got[k].flat[0]) == 10 + k for k in range(6))
    assert calls == ["area"]
    want = {11: (m1, _lat(1)), 13: (np.array([[0.0, 1.0], [0.5, 0.0]], dtype=np.float32), _lat(3)), 14: (m4, _lat(4))}
    seen = {}
    ev = fake.events
    for n, e in enumerate(ev):
        if e[0] == "start" and e[2] in want:
            nxt = ev[n + 1]
            assert nxt[0] == "inpaint" and nxt[1] == e[1], (e, nxt[:2])     # at once, the same slot
            seen[e[2]] = nxt
        if e[0] == "inpaint":
            prev = ev[n - 1]
            assert prev[0] == "start" and prev[1] == e[1] and prev[2] in want, (prev, e[:2])   # mask requests only
    assert sorted(seen) == sorted(want)
    for seed, (mask, known) in want.items():
        _, _, m, k = seen[seed]
        assert m.shape == (L, L) and m.dtype == np.float32 and np.array_equal(m, mask), seed
        assert np.array_equal(k, known), seed
    assert sum(e[0] == "inpaint" for e in ev) == 3


@pytest.mark.parametrize("shape", [(L,), (L, L + 1), (2, L, L), (8 * L, 4 * L), (1, 1, L, L), (3 * L, 3 * L)])
def test_a_mask_of_another_shape_is_refused_before_any_slot_is_touched(tsd_mod, shape):
    from tsd.serve import Request, SlotScheduler
    fake = FakeSession(B, STEPS, L)
    with pytest.raises(ValueError):
        list(SlotScheduler(fake, iter([Request(0, CTX, CTX, 1, 7.5, _lat(1), 1.0, np.ones(shape, dtype=np.float32))])))
    assert fake.events == []


def test_a_mask_without_latents_is_refused_before_any_slot_is_touched(tsd_mod):
    from tsd.serve import Request, SlotScheduler
    fake = FakeSession(B, STEPS, L)
    with pytest.raises(ValueError):
        list(SlotScheduler(fake, iter([Request(0, CTX, CTX, 1, mask=np.ones((L, L), dtype=np.float32))])))
    assert fake.events == []


def test_advance_makes_no_copy_from_the_host():
    """The per-slot scalars of both update kernels travel as kernel arguments: the text of tsd_session_advance, of the two functions it
    builds its tables and picks its update launch with, and of the slot launchers names no host-to-device copy (the GPU test counts the
    launches; a copy is not a launch)."""
    src = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "csrc", "session.cpp")).read()
    m = re.search(r'extern "C" int tsd_session_advance\(.*?\n}\n', src, re.S)
    tables = re.search(r'static int session_step_tables\(.*?\n}\n', src, re.S)
    update = re.search(r'static int session_update\(.*?\n}\n', src, re.S)
    assert m and tables and update and "session_step_tables(" in m.group(0) and "session_update(" in m.group(0)
    assert "launch_slot_update_blend" in update.group(0) and "launch_slot_update(" in update.group(0)
    for text in (m.group(0), tables.group(0), update.group(0)):
        assert "HostToDevice" not in text and "hipMemcpy(" not in text
    slots = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "csrc", "kernels_slots.hip")).read()
    assert "k_slot_update_blend" in slots and "hipMemcpy" not in slots
