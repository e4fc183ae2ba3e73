"""Slot sessions without a GPU: the C ABI's new symbols, and `tsd.serve.SlotScheduler` against a fake session that only counts."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS, B = 4, 3
STARTS = [0, 2, 0, 3, 1, 0, 2]
STRENGTH = {0: 1.0, 1: 0.75, 2: 0.5, 3: 0.25}   # generate's rule n - int(n * strength), inverted for n = 4
SLOT_SYMBOLS = ["tsd_session_slots_open", "tsd_session_slot_start", "tsd_session_advance", "tsd_session_slot_state",
                "tsd_session_slot_download", "tsd_session_slots_active"]


def test_slot_symbols_are_declared_exported_and_refuse_null(tsd_mod):
    from tsd._lib import TSD_E_ARG, ptr
    lib = tsd_mod._lib.lib()
    declared = tsd_mod._lib.declared_symbols()
    for name in SLOT_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    buf = np.zeros(77 * 768, dtype=np.float32)
    mask, idx, st = C.c_uint32(0), C.c_int(0), C.c_int(0)
    assert lib.tsd_session_slots_open(None) == TSD_E_ARG
    assert lib.tsd_session_slot_start(None, 0, ptr(buf), None, None, 0, 1, 0, 7.5) == TSD_E_ARG
    assert lib.tsd_session_advance(None, C.byref(mask)) == TSD_E_ARG
    assert lib.tsd_session_slot_state(None, 0, C.byref(idx), C.byref(st)) == TSD_E_ARG
    assert lib.tsd_session_slot_download(None, 0, ptr(buf)) == TSD_E_ARG
    assert lib.tsd_session_slots_active(None) < 0
    for name in ("slots_open", "slot_start", "advance", "slot_state", "slot_latents", "slots_active"):
        assert callable(getattr(tsd_mod.Session, name)), name
    shim = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "mojo_shim", "tsd_ffi.mojo")).read()
    for name in SLOT_SYMBOLS:
        assert f'"{name}"' in shim, name


class FakeSession:
    """The slot methods of `Session`, counting: no device, latents are the request's tag."""

    def __init__(self, B, num_steps):
        self.B, self.num_steps = B, num_steps
        self.index = [None] * B        # schedule index of an active slot
        self.tag = [None] * B
        self.advances = 0
        self.steps_taken = {}          # tag -> advances it was active in
        self.active_per_advance = []
        self.events = []               # ("start", b) / ("advance", active slots)

    def slot_start(self, b, context, uncond_context=None, latents=None, noise_at_start=False, seed=0, start_index=0, cfg_scale=7.5):
        assert 0 <= b < self.B and 0 <= start_index < self.num_steps
        assert self.index[b] is None, "the scheduler replaced a running request"
        assert noise_at_start == (latents is not None)
        self.index[b], self.tag[b] = start_index, seed
        self.steps_taken[seed] = 0
        self.events.append(("start", b))

    def advance(self):
        active = [b for b in range(self.B) if self.index[b] is not None]
        assert active, "advance with no active slot"
        self.advances += 1
        self.active_per_advance.append(len(active))
        self.events.append(("advance", tuple(active)))
        done = []
        for b in active:
            self.steps_taken[self.tag[b]] += 1
            self.index[b] += 1
            if self.index[b] == self.num_steps:
                self.index[b] = None
                done.append(b)
        self._last = {b: self.tag[b] for b in done}
        return done

    def slot_latents(self, b):
        return np.full((4, 1, 1), self._last[b], dtype=np.float32)


def _greedy_advances(starts, n, B):
    """Independent simulation of greedy filling: remaining steps per slot, refilled from the queue before every tick."""
    queue, slots, ticks, active_ticks = [n - s for s in starts], [0] * B, 0, 0
    while True:
        for b in range(B):
            if slots[b] == 0 and queue:
                slots[b] = queue.pop(0)
        busy = sum(1 for r in slots if r > 0)
        if not busy:
            return ticks, active_ticks
        ticks += 1
        active_ticks += busy
        slots = [max(r - 1, 0) for r in slots]


def test_scheduler_fills_greedily_and_reports_its_occupancy(tsd_mod):
    from tsd.serve import Request, SlotScheduler, start_index
    assert [start_index(STEPS, STRENGTH[s]) for s in STARTS] == STARTS and start_index(STEPS, None) == 0
    fake = FakeSession(B, STEPS)
    ctx = np.zeros((77, 768), dtype=np.float32)
    lat = np.zeros((4, 1, 1), dtype=np.float32)

    def requests():
        for k, s in enumerate(STARTS):
            yield Request(id=f"r{k}", context=ctx, uncond=ctx, seed=k, cfg_scale=7.5,
                          latents=None if s == 0 else lat, strength=None if s == 0 else STRENGTH[s])

    sched = SlotScheduler(fake, requests())
    got = list(sched)
    # every id exactly once, with its own latents
    assert sorted(i for i, _ in got) == sorted(f"r{k}" for k in range(len(STARTS)))
    for rid, la in got:
        assert la.shape == (4, 1, 1) and float(la.flat[0]) == float(rid[1:])
    # request k took exactly 4 - start_k advances
    assert fake.steps_taken == {k: STEPS - s for k, s in enumerate(STARTS)}
    # no advance ran with a free slot while the queue still held a request: replay the events, counting what was still queued
    started = 0
    for ev, what in fake.events:
        if ev == "start":
            started += 1
        else:
            assert len(what) == B or started == len(STARTS), (what, started)
    ticks, active_ticks = _greedy_advances(STARTS, STEPS, B)
    assert fake.advances == sched.advances == ticks
    assert sum(fake.active_per_advance) == active_ticks == sum(STEPS - s for s in STARTS)
    assert sched.active_ticks == active_ticks
    assert sched.occupancy == active_ticks / (B * ticks)
    print(f"[slots] {len(STARTS)} requests, B={B}: {ticks} advances, occupancy {sched.occupancy:.3f}")
