"""GPU: what the library does with device RESOURCES, read from its ledger (`tsd.device_ledger()`, csrc/device_ledger.h): every handle
gives back what it took, and the calls include/tsd.h and DESIGN.md promise "no allocation" for make none.

Every test takes snapshots of the ledger around work on a Context of its own and compares them - never an absolute value: the default
context of the run and other modules' fixtures are alive.  ALLOCS_TOTAL / FREES_TOTAL are monotone, so "this call allocated nothing" is
"neither moved".  Every test ends with FREES_UNKNOWN (a double or foreign release) and RELEASE_ERRORS where they were.

 1. context: eight create / destroy cycles, and one cycle that touches everything a context can own;
 2. profiling: a second identical pass creates no event, and the context's destroy releases them all;
 3. every model kind: the second forward allocates nothing; adapter snapshots come and go exactly; destroy while merged leaves nothing;
 4. Tiny-SD sessions (3 samplers x CFG x hoist): no step allocates or frees, whatever noise / seeds / inpainting / guidance rescale it
    runs with; a longer schedule replaces buffers; a session never holds more than the nine buffers its destroy lists; slot mode;
 5. a full-size session with ControlNet, IP-Adapter and IP-Adapter Plus: set_* allocate once, no step does;
 6. the 32-entry cache of resize tables: 34 sizes, eviction, and the evicted size rebuilt to the same bits;
 7. refusals leave the ledger where it was;
 8. `generate` / `generate_stream` close what they open, also when they raise;
 9. the communicator: a second init is refused, a context destroyed with a live communicator finalizes it.

Shapes are the smallest the paths accept: Tiny-SD at L = 8, B = 3, T = 77, 4 steps; full-size SD-1.5 at L = 16, B = 2, 3 steps; images
of 64 x 96 and smaller.  The counts each test prints are those of BASELINE.md section 4 ("Device resources").

Run on an MI355X against a build of the parent of the commit that added this file, with the ledger and nothing else applied: test 2
failed at its last assertion (EVENTS_LIVE 296 where the baseline is 2: the 294 events of ProfScope were never destroyed) and test 9 at
the second tsd_dist_init (it returned TSD_OK and overwrote the communicator).  Test 8's raising `generate` left its session open there
(by reading: the session was closed on the two normal ways out only)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ops, rng

pytestmark = pytest.mark.gpu
SEED, T = 1234, 77
N_TRAIN, STEPS = 1000, 4
B, L = 3, 8                     # Tiny-SD sessions (tests/test_gpu_slots.py)
FB, FL, FSTEPS = 2, 16, 3       # the full-size session (tests/test_gpu_ipplus.py)
LIVE = ("ALLOCS_LIVE", "BYTES_LIVE", "EVENTS_LIVE", "STREAMS_LIVE", "CTX_LIVE", "MODELS_LIVE", "SESSIONS_LIVE")
COUNTS = tuple(k for k in LIVE if k != "BYTES_LIVE")
SESSION_BUFFERS = 9             # tsd_session_destroy's list (tests/test_device_ledger_cpu.py holds the source to it)
SAMPLERS = [("ddpm", 0.0, "leading"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")]


def snap():
    import tsd
    return tsd.device_ledger()


def live(s, keys=LIVE):
    return {k: s[k] for k in keys}


def moved(a, b):
    """(allocations, frees) between two snapshots."""
    return b["ALLOCS_TOTAL"] - a["ALLOCS_TOTAL"], b["FREES_TOTAL"] - a["FREES_TOTAL"]


def quiet(what, fn, *args, **kw):
    """Run fn; it must neither allocate nor free."""
    a = snap()
    out = fn(*args, **kw)
    assert moved(a, snap()) == (0, 0), f"{what}: (allocations, frees) = {moved(a, snap())}"
    return out


@pytest.fixture(autouse=True)
def no_bad_release(gpu_ctx):
    a = snap()
    yield
    b = snap()
    assert (b["FREES_UNKNOWN"], b["RELEASE_ERRORS"]) == (a["FREES_UNKNOWN"], a["RELEASE_ERRORS"]), "a double / foreign release, or one HIP refused"
    assert b["ALLOCS_LIVE"] == b["ALLOCS_TOTAL"] - b["FREES_TOTAL"]


def mem_free():
    """hipMemGetInfo's free bytes through the HIP runtime the library is linked to; None when it cannot be asked.  Printed only."""
    try:
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
        free, total = C.c_size_t(0), C.c_size_t(0)
        return free.value if C.CDLL(path).hipMemGetInfo(C.byref(free), C.byref(total)) == 0 else None
    except Exception:  # noqa: BLE001
        return None


def tiny_inputs(nb, side=L):
    return (rng.normal(SEED, 3100, nb * 4 * side * side).reshape(nb, 4, side, side), rng.normal(SEED, 3101, nb * T * 768).reshape(nb, T, 768),
            np.repeat(ops.time_embedding(500.0).reshape(1, 320), nb, axis=0))


class hoist:
    def __init__(self, tsd_mod, ctx, on):
        self.lib, self.h, self.on = tsd_mod._lib.lib(), ctx.h, int(on)

    def __enter__(self):
        self.prev = self.lib.tsd_debug_set_session_hoist(self.h, self.on)

    def __exit__(self, *exc):
        self.lib.tsd_debug_set_session_hoist(self.h, self.prev)


# ---- 1. the context ----------------------------------------------------------------------------------------------------------------------
def test_context_cycles_leave_nothing(gpu_ctx, tsd_mod):
    made = []
    for cycle in range(8):
        a = snap()
        c = tsd_mod.Context(gpu_ctx.device)
        m = snap()
        c.close()
        b = snap()
        assert live(b) == live(a), cycle
        assert {k: m[k] - a[k] for k in COUNTS} == dict(ALLOCS_LIVE=2, EVENTS_LIVE=2, STREAMS_LIVE=1, CTX_LIVE=1, MODELS_LIVE=0, SESSIONS_LIVE=0)
        made.append(moved(a, b))
    print(f"[lifetime] context create / destroy: (allocations, frees) per cycle {made[0]}, {m['BYTES_LIVE'] - a['BYTES_LIVE']} bytes held")
    assert made == [made[0]] * 8 and made[0] == (2, 2)


def test_fat_context_cycle_leaves_nothing(gpu_ctx, tsd_mod):
    """One context made to own everything it can: the arena grown twice, the staging buffer grown, the split-K flags, profiling events,
    three resize tables - and a model and a session on it.  After the destroys every live count is where it was."""
    lib = tsd_mod._lib.lib()
    free0 = mem_free()
    a = snap()
    c = tsd_mod.Context(gpu_ctx.device)
    made = snap()
    ip = tsd_mod.IPAdapter(seed=3, ctx=c)                        # a seeded init stages its largest parameter: the staging buffer ...
    small = snap()
    d = tsd_mod.Diffusion(seed=SEED, ctx=c)                      # ... which a model with a larger one replaces
    s0 = snap()
    assert moved(made, small) == (2, 0) and moved(small, s0) == (2, 1) and s0["BYTES_LIVE"] > small["BYTES_LIVE"], "blob + staging, then blob + staging grown"
    assert lib.tsd_debug_gemm_record(c.h, 1) >= 0
    d.forward(*tiny_inputs(1))                                   # the arena (and the model's derived buffers, and the split-K flags)
    n_rec = lib.tsd_debug_gemm_record(c.h, 0)
    import gemm_ref as G
    ways, desc, plan = 0, np.zeros(G.COUNT, np.int64), np.zeros(G.GP["COUNT"], np.int64)
    i64p = C.POINTER(C.c_int64)
    for i in range(n_rec):
        assert lib.tsd_debug_gemm_recorded(c.h, i, desc.ctypes.data_as(i64p), len(desc)) == G.COUNT
        assert lib.tsd_debug_gemm_plan(c.h, desc.ctypes.data_as(i64p), len(desc), -1, plan.ctypes.data_as(i64p)) == 0
        ways = max(ways, int(plan[G.GP["WAYS"]]))
    assert n_rec > 20 and ways > 1, "no launch of this forward runs split-K: the context has no hand-off flags to free"
    s1 = snap()
    d.forward(*tiny_inputs(2, 16))                               # a larger plan: the arena is replaced
    s2 = snap()
    assert moved(s0, s1)[0] >= 3 and moved(s1, s2)[1] >= 1 and s2["BYTES_LIVE"] > s1["BYTES_LIVE"] and s2["ALLOCS_LIVE"] == s1["ALLOCS_LIVE"]
    d.forward(*tiny_inputs(3, 24))                               # ... twice
    s3 = snap()
    assert moved(s2, s3) == (1, 1) and s3["BYTES_LIVE"] > s2["BYTES_LIVE"]
    weights = sorted((int(np.prod(sp[1])), i) for i, sp in enumerate(d.model.specs) if sp[2] and len(sp[1]) >= 2)
    for numel, i in (weights[0], weights[len(weights) // 2]):    # two adapter snapshots; the merges run in the staging buffer as it is
        shape = d.model.specs[i][1]
        d.model.lora_add(i, np.zeros((shape[0], 2), np.float32), np.zeros((2, numel // shape[0]), np.float32), 1.0)
    s4 = snap()
    assert moved(s3, s4) == (2, 0), moved(s3, s4)
    c.profile_begin()
    d.forward(*tiny_inputs(1))
    launches = sum(n for _, n in c.profile_end().values())
    s5 = snap()
    assert s5["EVENTS_LIVE"] - s4["EVENTS_LIVE"] >= 2 and launches > 20
    for H, W in ((8, 8), (64, 96), (33, 20)):
        tsd_mod.clip_image_patches(np.full((3, H, W), 100.0, np.float32), ctx=c)
    s6 = snap()
    assert s6["ALLOCS_LIVE"] - s5["ALLOCS_LIVE"] == 3
    sess = tsd_mod.Session(d.model, None, 1, L, T, cfg=False)
    sess.set_schedule(N_TRAIN, 2, 0)
    lat, cx, _ = tiny_inputs(1)
    sess.upload(lat, cx, None, None)
    sess.set_seeds([5])
    sess.step(0)
    s7 = snap()
    print(f"[lifetime] fat context: {s7['ALLOCS_LIVE'] - a['ALLOCS_LIVE']} allocations, {s7['BYTES_LIVE'] - a['BYTES_LIVE']} bytes, "
          f"{s7['EVENTS_LIVE'] - a['EVENTS_LIVE']} events live before the destroys; {moved(a, s7)[0]} allocations made")
    sess.close()
    d.model.close()                                              # with two adapters merged
    ip.model.close()
    c.close()
    assert live(snap()) == live(a)
    free1 = mem_free()
    print(f"[lifetime] hipMemGetInfo free bytes before / after the fat cycle: {free0} / {free1} (printed, not asserted: the device is shared)")


# ---- 2. profiling ------------------------------------------------------------------------------------------------------------------------
def test_profiling_events_are_reused_and_released(gpu_ctx, tsd_mod):
    a = snap()
    c = tsd_mod.Context(gpu_ctx.device)
    d = tsd_mod.Diffusion(seed=SEED, ctx=c)
    x = tiny_inputs(2)
    d.forward(*x)
    s0 = snap()
    passes = []
    for _ in range(2):
        c.profile_begin()
        d.forward(*x)
        prof = c.profile_end()
        passes.append((snap(), sum(n for _, n in prof.values())))
    (s1, n1), (s2, n2) = passes
    made = s1["EVENTS_LIVE"] - s0["EVENTS_LIVE"]
    print(f"[lifetime] profiling a Tiny-SD forward: {n1} launches, {made} events created by the first pass, {s2['EVENTS_LIVE'] - s1['EVENTS_LIVE']} by the second")
    assert n1 == n2 > 20 and made >= 2 and made % 2 == 0 and made <= 2 * n1
    assert s2["EVENTS_LIVE"] == s1["EVENTS_LIVE"], "a second identical pass created events"
    assert moved(s0, s2) == (0, 0), "profiling allocated device memory"
    quiet("a forward after profiling", d.forward, *x)
    d.model.close()
    c.close()
    assert live(snap()) == live(a), "the context's destroy left profiling events (or anything else) behind"


# ---- 3. models ---------------------------------------------------------------------------------------------------------------------------
def _kinds():
    from tsd.model import KINDS
    return sorted(KINDS, key=KINDS.get)


NO_ADAPTERS = ("controlnet_sd15", "controlnet_sd15_torch", "ip_adapter_sd15", "ip_adapter_plus_sd15", "clip_vision_h")


def _module_and_forward(tsd_mod, kind, c):
    """(wrapper, forward()) of one model of `kind` on context c, at the smallest shape its entry accepts."""
    g = np.random.default_rng(7)
    small = lambda *shape: (0.5 * g.standard_normal(shape)).astype(np.float32)  # noqa: E731
    if kind.startswith("diffusion"):
        m = tsd_mod.Diffusion(seed=5, ctx=c, variant=kind)
        side = L if kind == "diffusion" else FL
        args = (small(1, 4, side, side), small(1, T, m.model.context_width), ops.time_embedding(500.0).reshape(1, 320))
        return m, lambda: m.forward(*args)
    if kind.startswith("decoder"):
        m = tsd_mod.Decoder(seed=5, ctx=c, variant=kind)
        x = small(1, 4, 8, 8)
        return m, lambda: m.forward(x)
    if kind.startswith("encoder"):
        m = tsd_mod.Encoder(seed=5, ctx=c, variant=kind)
        x, nz = small(1, 3, 64, 64), small(1, 4, 8, 8)
        return m, lambda: m.forward(x, nz)
    if kind == "clip_vision_h":
        m = tsd_mod.CLIPVision(seed=5, ctx=c)
        img = (128.0 + 40.0 * small(3, 32, 48)).astype(np.float32)
        return m, lambda: m.forward(img, hidden=True)
    if kind.startswith("clip"):
        m = tsd_mod.CLIP(seed=5, ctx=c, variant=kind)
        return m, lambda: m.forward(np.array([1, 5, 9, 2, 7], np.int32))
    if kind.startswith("controlnet"):
        m = tsd_mod.ControlNet(seed=5, ctx=c, variant=kind)
        args = (small(1, 4, FL, FL), small(1, T, 768), ops.time_embedding(500.0).reshape(1, 320), np.abs(small(1, 3, 8 * FL, 8 * FL)))
        return m, lambda: m.forward(*args)
    m = tsd_mod.IPAdapter(seed=5, ctx=c, variant=kind)
    if kind == "ip_adapter_plus_sd15":
        h = small(1, 5, 1280)
        return m, lambda: m.resample(h)
    e = small(1, 1024)
    return m, lambda: m.project(e)


def test_the_kinds_under_test_are_the_kinds_the_library_lists(gpu_ctx, tsd_mod):
    from tsd.model import KINDS
    listed = {k for k in range(0, 64) if tsd_mod._lib.lib().tsd_model_param_count(k) > 0}
    assert listed == set(KINDS.values()) and len(KINDS) == len(listed) == 16
    assert all(k in KINDS for k in NO_ADAPTERS)


@pytest.mark.parametrize("kind", _kinds())
def test_model_lifetime(gpu_ctx, tsd_mod, kind):
    a = snap()
    c = tsd_mod.Context(gpu_ctx.device)
    w, forward = _module_and_forward(tsd_mod, kind, c)
    m = w.model
    s0 = snap()
    forward()
    s1 = snap()
    quiet(f"{kind}: the second forward", forward)
    line = f"[lifetime] {kind}: create {moved(a, s0)[0] - 2} allocation(s), first forward {moved(s0, s1)} (allocations, frees), second (0, 0)"
    if kind in NO_ADAPTERS:
        from tsd._lib import lib, ptr
        one = np.zeros((1, 1), np.float32)
        assert quiet(f"{kind}: a refused lora_add", lib().tsd_model_lora_add, m.h, 0, 0, 1, ptr(one), ptr(one), 1, 1.0) == tsd_mod._lib.TSD_E_ARG
    else:
        weights = sorted((int(np.prod(sp[1])), i) for i, sp in enumerate(m.specs) if sp[2] and len(sp[1]) >= 2)
        (n0, p0), (n1, p1) = weights[0], weights[1]

        def adapter(i, numel, seed):
            rows = m.specs[i][1][0]
            g = np.random.default_rng(seed)
            return i, (0.01 * g.standard_normal((rows, 2))).astype(np.float32), (0.01 * g.standard_normal((2, numel // rows))).astype(np.float32), 0.5
        m.lora_add(*adapter(p0, n0, 1))                        # once through everything below, so that the context's staging buffer
        m.lora_add(*adapter(p1, n1, 1))                        # has its size: what is counted afterwards is the model's alone
        m.lora_clear()
        m.set_param(p0, m.get_param(p0))
        forward()
        base = snap()
        m.lora_add(*adapter(p0, n0, 2))
        m.lora_add(*adapter(p1, n1, 3))
        s2 = snap()
        assert moved(base, s2) == (2, 0) and m.lora_count == 2, "two adapted parameters: exactly two snapshots"
        quiet(f"{kind}: a stacked add", m.lora_add, *adapter(p0, n0, 4))
        m.lora_clear()
        s3 = snap()
        assert moved(s2, s3) == (0, 2) and live(s3) == live(base) and m.lora_count == 0
        m.lora_add(*adapter(p0, n0, 5))
        forward()
        m.lora_clear()
        forward()
        s4 = snap()
        assert s4["ALLOCS_LIVE"] == base["ALLOCS_LIVE"], "add -> forward -> clear -> forward holds another allocation count than before"
        m.lora_add(*adapter(p0, n0, 6))
        m.lora_add(*adapter(p1, n1, 7))
        s5 = snap()
        m.set_param(p0, m.get_param(p0))                       # the merged value is the new base: its snapshot goes
        s6 = snap()
        assert moved(s5, s6) == (0, 1) and m.lora_count == 1
        line += f"; derived rebuild after a merge {moved(s3, s4)}"
    print(line)
    m.close()                                                    # the adapter kinds: with one parameter still merged
    c.close()
    assert live(snap()) == live(a), f"{kind}: something outlives the model and its context"


# ---- 4. Tiny-SD sessions -----------------------------------------------------------------------------------------------------------------
class World:
    pass


@pytest.fixture(scope="module")
def tiny(gpu_ctx, tsd_mod):
    """A context of this module's own with a Tiny-SD UNet on it, warmed: arena, staging, derived buffers and split-K flags are in place."""
    a = snap()
    w = World()
    w.ctx = tsd_mod.Context(gpu_ctx.device)
    w.unet = tsd_mod.Diffusion(seed=SEED, ctx=w.ctx)
    w.lat, w.cx, _ = tiny_inputs(B)
    w.ucx = rng.normal(SEED, 3102, B * T * 768).reshape(B, T, 768)
    w.unet.forward(*tiny_inputs(2 * B))
    for on in (1, 0):
        with hoist(tsd_mod, w.ctx, on):
            s = tsd_mod.Session(w.unet.model, None, B, L, T, cfg=True)
            s.set_schedule(N_TRAIN, STEPS + 2, 0)
            s.upload(w.lat, w.cx, w.ucx, None)
            s.set_seeds([1, 2, 3])
            s.step(0)
            s.close()
    yield w
    w.unet.model.close()
    w.ctx.close()
    assert live(snap()) == live(a), "the Tiny-SD world of this module left something behind"


def _steps(s, what, first=0):
    for i in range(first, s.num_steps):
        quiet(f"{what}, step {i}", s.step, i)


@pytest.mark.parametrize("on", [1, 0], ids=["hoist", "nohoist"])
@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_no_step_of_a_session_allocates_or_frees(gpu_ctx, tsd_mod, tiny, sampler, cfg, on):
    a = snap()
    ucx = tiny.ucx if cfg else None
    noise = rng.normal(SEED, 3103, (STEPS + 2) * B * 4 * L * L).reshape(STEPS + 2, B, 4, L, L)
    mask = (rng.uniform(SEED, 3104, B * L * L, 1.0) > 0).astype(np.float32).reshape(B, L, L)
    held = []

    def holds(s):
        n = snap()["ALLOCS_LIVE"] - a["ALLOCS_LIVE"]           # the warmed context replaces its arena / staging, it never adds one
        held.append(n)
        assert 1 <= n <= SESSION_BUFFERS, f"the session holds {n} allocations; its destroy lists {SESSION_BUFFERS}"
    with hoist(tsd_mod, tiny.ctx, on):
        s = tsd_mod.Session(tiny.unet.model, None, B, L, T, cfg=cfg)
        assert moved(a, snap()) == (1, 0)                        # the state block
        s.set_sampler(*sampler)
        s.set_schedule(N_TRAIN, STEPS, 0)
        s.upload(tiny.lat, tiny.cx, ucx, noise[:STEPS])
        holds(s)
        _steps(s, "noise tensor")
        s.upload(tiny.lat, tiny.cx, ucx, None)
        s.set_seeds([11, 12, 13])
        quiet("seed_latents", s.seed_latents)
        _steps(s, "seeds")
        s.upload(tiny.lat, tiny.cx, ucx, None)
        s.set_seeds([11, 12, 13])
        s.add_noise_seeded(0)
        s.set_inpaint(mask, tiny.lat, seeded=True)
        _steps(s, "seeded inpainting")
        s.upload(tiny.lat, tiny.cx, ucx, noise[:STEPS])
        s.set_inpaint(mask, tiny.lat, noise[0])
        _steps(s, "inpainting with a noise tensor")
        n_steps = 4 * STEPS
        if cfg:
            s.upload(tiny.lat, tiny.cx, ucx, noise[:STEPS])
            s.set_guidance_rescale(0.7)
            _steps(s, "guidance rescale")
            n_steps += STEPS
        quiet("download", s.latents)
        holds(s)
        before = snap()
        s.set_schedule(N_TRAIN, STEPS + 2, 0)                    # a longer schedule: the noise buffer (and the time table) are replaced
        s.upload(tiny.lat, tiny.cx, ucx, noise)
        after = snap()
        grown = moved(before, after)
        assert after["ALLOCS_LIVE"] == before["ALLOCS_LIVE"] and grown[0] == grown[1] >= 1, grown
        assert after["BYTES_LIVE"] > before["BYTES_LIVE"]
        holds(s)
        _steps(s, "the longer schedule")
        s.close()
    print(f"[lifetime] session {sampler[0]} cfg={int(cfg)} hoist={on}: {held[0]} allocations after upload, {held[-1]} after the longer one "
          f"({grown[0]} replaced), 0 in {n_steps + STEPS + 2} steps")
    assert live(snap()) == live(a)


@pytest.mark.parametrize("on", [1, 0], ids=["hoist", "nohoist"])
@pytest.mark.parametrize("cfg", [False, True], ids=["nocfg", "cfg"])
def test_slot_mode_allocates_nothing_once_open(gpu_ctx, tsd_mod, tiny, cfg, on):
    """The first slots_open() of a session sizes what upload() would have (context K / V^T, time table, time rows); from then on a second
    slots_open(), every slot_start, advance, refill and slot inpainting request allocate nothing."""
    a = snap()
    req = [dict(ctx=tiny.cx[k], uctx=tiny.ucx[k] if cfg else None, seed=100 + k) for k in range(B)]
    mask = np.zeros((L, L), np.float32)
    mask[:, : L // 2] = 1.0
    with hoist(tsd_mod, tiny.ctx, on):
        s = tsd_mod.Session(tiny.unet.model, None, B, L, T, cfg=cfg)
        s.set_schedule(N_TRAIN, STEPS, 0)
        s.slots_open()
        opened = snap()
        n_open = opened["ALLOCS_LIVE"] - a["ALLOCS_LIVE"]
        assert 1 <= n_open <= SESSION_BUFFERS and (on == 1) == (n_open > 1)
        quiet("a second slots_open", s.slots_open)
        for k in range(B):
            quiet(f"slot_start {k}", s.slot_start, k, req[k]["ctx"], req[k]["uctx"], seed=req[k]["seed"])
            if k == 0:
                quiet("advance", s.advance)                      # slot 0 runs one step ahead of the others
        done, ticks = [], 0
        while s.slots_active():
            finished = quiet("advance", s.advance)
            ticks += 1
            for k in finished:
                quiet("slot download", s.slot_latents, k)
                if not done:                                     # the first slot to finish is refilled with an inpainting img2img request
                    quiet("refill", s.slot_start, k, req[1]["ctx"], req[1]["uctx"], latents=tiny.lat[k], noise_at_start=True, seed=7, start_index=2)
                    quiet("slot_set_inpaint", s.slot_set_inpaint, k, mask, tiny.lat[k])
                done.append(k)
            assert ticks < 4 * STEPS
        assert sorted(done) == [0, 0, 1, 2] and moved(opened, snap()) == (0, 0)
        s.close()
    print(f"[lifetime] slot session cfg={int(cfg)} hoist={on}: {n_open} allocations after slots_open, 0 in {ticks + 1} advances, 4 submits and a slot inpainting request")
    assert live(snap()) == live(a)


# ---- 5. the full-size session ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(gpu_ctx, tsd_mod):
    """A context of this module's own with the full-size SD-1.5 UNet, a ControlNet, both IP-Adapters and the CLIP vision encoder, each
    warmed by a forward so that its derived buffers exist.  Torn down session first, models next, the context last: nothing may remain."""
    a = snap()
    w = World()
    w.ctx = c = tsd_mod.Context(gpu_ctx.device)
    w.unet = tsd_mod.Diffusion(seed=SEED, ctx=c, variant="diffusion_sd15")
    w.cn = tsd_mod.ControlNet(seed=2, ctx=c)
    w.ip = tsd_mod.IPAdapter(seed=3, ctx=c)
    w.plus = tsd_mod.IPAdapter(seed=4, ctx=c, variant="ip_adapter_plus_sd15")
    w.enc = tsd_mod.CLIPVision(seed=11, ctx=c)
    w.lat = rng.normal(7, 3200, FB * 4 * FL * FL).reshape(FB, 4, FL, FL)
    w.cx = rng.normal(7, 3201, FB * T * 768).reshape(FB, T, 768)
    w.ucx = rng.normal(7, 3202, FB * T * 768).reshape(FB, T, 768)
    w.hint = (rng.uniform(7, 3203, 3 * 64 * FL * FL, 0.5) + np.float32(0.5)).reshape(3, 8 * FL, 8 * FL)
    w.img = ((rng.uniform(7, 3204, 3 * 64 * 48, 0.5) + np.float32(0.5)) * np.float32(255.0)).reshape(3, 64, 48)
    temb = np.repeat(ops.time_embedding(500.0).reshape(1, 320), FB, axis=0)
    emb, hid = w.enc.forward(w.img, hidden=True)
    w.tok = w.ip.project(np.repeat(emb[None], FB, axis=0))
    w.tok16 = w.plus.resample(np.repeat(hid[None], FB, axis=0))
    assert w.tok.shape == (FB, 4, 768) and w.tok16.shape == (FB, 16, 768)
    w.unet.forward(w.lat, w.cx, temb, control=w.cn, hint=w.hint, ip_adapter=w.plus, ip_tokens=w.tok16)
    w.session = None
    yield w
    if w.session is not None:                                    # the session test closes its session and checks that destroy itself; one
        w.session.close()                                        # that failed half-way still goes before the models (close is idempotent)
    for m in (w.enc, w.plus, w.ip, w.cn, w.unet):
        m.model.close()
    w.ctx.close()
    assert live(snap()) == live(a), "the full-size world of this module left something behind"


def test_each_full_size_kind_is_created_and_destroyed_once(gpu_ctx, tsd_mod):
    a = snap()
    c = tsd_mod.Context(gpu_ctx.device)
    tsd_mod.Model("ip_adapter_sd15", ctx=c, seed=1).close()      # the context has its staging buffer: a seeded init of a larger model replaces it
    per_kind = {}
    for kind in ("diffusion_sd15", "diffusion_sd15_torch", "diffusion_sd2", "controlnet_sd15", "controlnet_sd15_torch", "clip_vision_h", "clip_sd2"):
        s0 = snap()
        m = tsd_mod.Model(kind, ctx=c, seed=1)
        s1 = snap()
        m.close()
        s2 = snap()
        assert live(s2, COUNTS) == live(s0, COUNTS) and moved(s1, s2) == (0, 1), kind
        per_kind[kind] = (s1["ALLOCS_LIVE"] - s0["ALLOCS_LIVE"], s1["BYTES_LIVE"] - s2["BYTES_LIVE"])
    print(f"[lifetime] full-size kinds, (allocations, bytes) of the model: {per_kind}")
    assert all(v[0] == 1 and v[1] > 100 << 20 for v in per_kind.values())
    c.close()
    assert live(snap()) == live(a)


def test_full_size_session_with_control_and_adapters(gpu_ctx, tsd_mod, full):
    w = full
    a = snap()
    s = w.session = tsd_mod.Session(w.unet.model, None, FB, FL, T, cfg=True)
    s.set_sampler("ddim", 0.0, "leading")
    s.set_schedule(N_TRAIN, FSTEPS, 0)
    s.upload(w.lat, w.cx, w.ucx, None)
    s0 = snap()
    s.set_control(w.cn, w.hint, scale=0.8, first_step=1, last_step=1)
    s1 = snap()
    assert moved(s0, s1)[0] >= 1 and s.control_active
    quiet("set_control again, same shapes", s.set_control, w.cn, w.hint, scale=0.8, first_step=1, last_step=1)
    utok = w.ip.project(np.zeros((FB, 1024), np.float32))
    s2 = snap()
    s.set_ip_adapter(w.ip, w.tok, utok, scale=0.7, first_step=1, last_step=2)
    s3 = snap()
    assert moved(s2, s3)[0] >= 1 and s.ip_adapter_active
    quiet("set_ip_adapter again, same shapes", s.set_ip_adapter, w.ip, w.tok, utok, scale=0.7, first_step=1, last_step=2)
    _steps(s, "ControlNet window [1, 1], IP-Adapter window [1, 2]")     # step 0 outside both, 1 inside both, 2 inside the adapter's
    assert np.isfinite(s.latents()).all()
    utok16 = w.plus.resample(np.zeros((FB, 5, 1280), np.float32))
    s4 = snap()
    s.set_ip_adapter(w.plus, w.tok16, utok16, scale=0.7, first_step=0, last_step=1)
    s5 = snap()
    quiet("set_ip_adapter (plus) again", s.set_ip_adapter, w.plus, w.tok16, utok16, scale=0.7, first_step=0, last_step=1)
    s.upload(w.lat, w.cx, w.ucx, None)
    _steps(s, "ControlNet window [1, 1], IP-Adapter Plus window [0, 1]")
    s.set_control(None)
    s.set_ip_adapter(None)
    s.upload(w.lat, w.cx, w.ucx, None)
    _steps(s, "control and adapter off")
    held = snap()["ALLOCS_LIVE"] - a["ALLOCS_LIVE"]
    print(f"[lifetime] full-size session: set_control {moved(s0, s1)}, set_ip_adapter {moved(s2, s3)}, plus {moved(s4, s5)} (allocations, frees); "
          f"{held} allocations held; 0 in {3 * FSTEPS} steps")
    assert 1 <= held <= SESSION_BUFFERS
    # the image-prompt entries at a shape they have seen
    hid = np.zeros((FB, 257, 1280), np.float32)
    w.plus.resample(hid)
    quiet("resample, second call", w.plus.resample, hid)
    quiet("project, second call", w.ip.project, np.zeros((FB, 1024), np.float32))
    quiet("CLIPVision.forward, second call", w.enc.forward, w.img, hidden=True)
    tsd_mod.clip_image_patches(w.img, ctx=w.ctx)
    quiet("clip_image_patches, second call", tsd_mod.clip_image_patches, w.img, ctx=w.ctx)
    s.close()                                                    # the session first; the module's fixture destroys the models, then the context
    assert live(snap(), COUNTS) == live(a, COUNTS), "the session's destroy left something of it behind"


# ---- 6. the cache of resize tables -------------------------------------------------------------------------------------------------------
def test_resize_table_cache_evicts_and_rebuilds_the_same_bits(gpu_ctx, tsd_mod):
    import clipvision_ref as R
    a = snap()
    c = tsd_mod.Context(gpu_ctx.device)
    img = lambda W: np.random.default_rng(W).uniform(0.0, 255.0, size=(3, 8, W)).astype(np.float32)  # noqa: E731
    first = tsd_mod.clip_image_patches(img(8), ctx=c)
    base = snap()                                                # the context's arena and one table
    most = 1
    for W in range(9, 42):                                       # 34 distinct sizes with the first
        tsd_mod.clip_image_patches(img(W), ctx=c)
        now = snap()
        tables = now["ALLOCS_LIVE"] - base["ALLOCS_LIVE"] + 1    # the arena is replaced when it grows, never added to
        assert tables == min(W - 7, 32), (W, tables)
        most = max(most, tables)
    made, freed = moved(base, snap())
    assert most == 32 and freed >= 2, "the eviction branch was not reached"
    quiet("a cached size", tsd_mod.clip_image_patches, img(41), ctx=c)
    before = snap()
    again = tsd_mod.clip_image_patches(img(8), ctx=c)            # evicted by the 33rd size
    assert moved(before, snap()) == (1, 1), "the first size was still cached (or its rebuild is not one table for one)"
    assert np.array_equal(again.view(np.uint16), first.view(np.uint16)), "the rebuilt table gives other bits than the evicted one"
    ref, bnd = R.bound(img(8))
    ratio = np.abs(again[:, :R.PATCH_K].astype(np.float64) - ref) / bnd
    print(f"[lifetime] resize tables: 34 sizes, at most {most} live, {made} built and {freed} freed; 8x8 after its eviction: worst |err| / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0 and (again[:, R.PATCH_K:].view(np.uint16) == 0).all()
    c.close()
    assert live(snap()) == live(a)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ledger_where_it_was(gpu_ctx, tsd_mod, tiny, full):
    import clipvision_ref as R
    from tsd._lib import f32, lib, ptr, vp
    E = tsd_mod._lib
    a = snap()
    c2 = tsd_mod.Context(gpu_ctx.device)
    dec = tsd_mod.Model("decoder", ctx=c2, seed=77)
    cn2 = tsd_mod.ControlNet(seed=2, ctx=c2)
    ip2 = tsd_mod.IPAdapter(seed=3, ctx=c2)
    ones = np.ones((3, 4), np.float32), np.ones((4, 128 * 9), np.float32)
    dec.lora_add("l26.kernel", ones[0], ones[1], 1e-3)           # sizes c2's staging buffer for the refused merge below
    dec.lora_clear()
    tsd_mod.clip_image_patches(np.zeros((3, 8, 64), np.float32), ctx=c2)
    rc, _, info = R.run(c2, np.zeros((1, 3, 8, 8), np.float32))  # a replay run that succeeds: its guarded operands are gone afterwards
    assert rc == 0
    s = tsd_mod.Session(full.unet.model, None, FB, FL, T, cfg=False)
    s.set_sampler("ddim", 0.0, "leading")
    s.set_schedule(N_TRAIN, FSTEPS, 0)
    s.upload(full.lat, full.cx, None, None)
    before = snap()

    def code(fn, *args, **kw):
        with pytest.raises(tsd_mod.TsdError) as e:
            fn(*args, **kw)
        return e.value.code
    assert code(tsd_mod.Session, tiny.unet.model, None, B, 12, T) == E.TSD_E_SHAPE               # a bad shape
    assert code(tsd_mod.Session, tiny.unet.model, dec, B, L, T) == E.TSD_E_ARG                   # a decoder of another context
    assert code(tsd_mod.Model, 99, ctx=c2) == E.TSD_E_ARG                                        # an unknown kind
    i26 = dec.param_index("l26.kernel")
    assert lib().tsd_model_lora_add(dec.h, i26, 0, 3, ptr(f32(ones[0])), ptr(f32(ones[1])), 0, 1.0) == E.TSD_E_ARG       # rank 0
    assert lib().tsd_model_lora_add(dec.h, i26, 0, 3, ptr(f32(ones[0])), ptr(f32(ones[1])), 1025, 1.0) == E.TSD_E_ARG
    assert code(dec.lora_add, "l26.kernel", ones[0], ones[1], 1e6) == E.TSD_E_NONFINITE and dec.lora_count == 0
    assert code(s.set_control, cn2, full.hint) == E.TSD_E_ARG and not s.control_active
    assert code(s.set_ip_adapter, ip2, full.tok[:, :, :]) == E.TSD_E_ARG and not s.ip_adapter_active
    out = np.zeros((1, 16, 768), np.float32)
    for S in (0, 1025):
        assert lib().tsd_ip_adapter_resample(full.plus.model.h, ptr(np.zeros((1, 1025, 1280), np.float32)), 1, S, ptr(out)) == E.TSD_E_SHAPE
    assert code(tsd_mod.clip_image_patches, np.zeros((3, 7, 64), np.float32), ctx=c2) == E.TSD_E_SHAPE
    assert R.run(c2, np.zeros((1, 3, 7, 64), np.float32), unsizable_ok=True)[0] == E.TSD_E_SHAPE
    i64p = C.POINTER(C.c_int64)
    for fn, extra in (("tsd_debug_gemm_run", (-1,)), ("tsd_debug_norm_run", ()), ("tsd_debug_attn_run", ()), ("tsd_debug_chain_run", ()),
                      ("tsd_debug_elem_run", ()), ("tsd_debug_ip_attn_run", ()), ("tsd_debug_image_patches_run", ())):
        d, ext, inf = np.zeros(1, np.int64), np.zeros(32, np.int64), np.zeros(32, np.int64)      # one field, and no known version in it
        ins, outs = (vp * 32)(), (vp * 32)()
        rc = getattr(lib(), fn)(c2.h, d.ctypes.data_as(i64p), 1, *extra, ins, outs, ext.ctypes.data_as(i64p), inf.ctypes.data_as(i64p))
        assert rc in (E.TSD_E_ARG, E.TSD_E_SHAPE), (fn, rc)
    after = snap()
    assert live(after, COUNTS) == live(before, COUNTS) and after["BYTES_LIVE"] >= before["BYTES_LIVE"], (live(before), live(after))
    print(f"[lifetime] refusals: (allocations, frees) {moved(before, after)}, {after['BYTES_LIVE'] - before['BYTES_LIVE']} bytes of staging / arena growth")
    assert moved(before, after)[0] == moved(before, after)[1]    # only a replaced arena or staging buffer
    s.close()
    for m in (ip2.model, cn2.model, dec):
        m.close()
    c2.close()
    assert live(snap()) == live(a)


# ---- 8. the Python level -----------------------------------------------------------------------------------------------------------------
def test_generate_and_generate_stream_close_what_they_open(gpu_ctx, tsd_mod, tiny, full):
    keys = ("SESSIONS_LIVE", "MODELS_LIVE", "ALLOCS_LIVE", "EVENTS_LIVE", "STREAMS_LIVE", "CTX_LIVE")
    a = snap()

    def twice(what, fn):
        fn()
        s1 = snap()
        fn()
        s2 = snap()
        assert live(s2, keys) == live(s1, keys), what
        assert s1["SESSIONS_LIVE"] == a["SESSIONS_LIVE"] and s1["MODELS_LIVE"] == a["MODELS_LIVE"], what
        print(f"[lifetime] {what}: (allocations, frees) of the second call {moved(s1, s2)}")
    kw = dict(uncond_context=tiny.ucx[:2], cfg=True, inference_steps=2, L=L, return_latents=True, seeds=[1, 2])
    twice("generate", lambda: tsd_mod.generate(tiny.unet, None, tiny.cx[:2], **kw))
    fkw = dict(uncond_context=full.ucx, cfg=True, inference_steps=2, L=FL, return_latents=True, seeds=[3, 4], strength=1.0)
    twice("generate with an image prompt", lambda: tsd_mod.generate(full.unet, None, full.cx, ip_adapter=full.ip, ip_image=full.img, image_encoder=full.enc, **fkw))
    twice("generate with an image prompt (plus)", lambda: tsd_mod.generate(full.unet, None, full.cx, ip_adapter=full.plus, ip_image=full.img, image_encoder=full.enc, **fkw))
    reqs = lambda: [tsd_mod.Request(k, tiny.cx[k % B], tiny.ucx[k % B], 50 + k) for k in range(4)]  # noqa: E731
    twice("generate_stream", lambda: list(tsd_mod.generate_stream(tiny.unet, None, reqs(), 2, L, inference_steps=2, return_latents=True)))
    # a call that raises after its session exists closes it: a noise tensor of the wrong shape is refused by upload()
    before = snap()
    with pytest.raises(ValueError):
        tsd_mod.generate(tiny.unet, None, tiny.cx[:2], uncond_context=tiny.ucx[:2], inference_steps=2, L=L, noise=np.zeros((1, 2, 4, L, L), np.float32))
    gen = tsd_mod.generate_stream(tiny.unet, None, reqs(), 2, L, inference_steps=2, return_latents=True)
    next(gen)
    gen.close()                                                  # a stream abandoned half-way
    assert live(snap(), keys) == live(before, keys), "a generate that raised, or an abandoned stream, left its session behind"


# ---- 9. the communicator -----------------------------------------------------------------------------------------------------------------
def test_second_dist_init_is_refused_and_destroy_finalizes(gpu_ctx, tsd_mod):
    """One rank, as tests/test_gpu_models.py::test_native_rccl_path_single_rank.  What RCCL itself allocates on the device for a
    communicator is outside the ledger (the library makes those calls in librccl, not through its wrappers): "zero" below is the
    library's own resources, and that the destroy of a context with a live communicator succeeds and leaves no handle."""
    from tsd._lib import check, lib
    E = tsd_mod._lib
    a = snap()
    c = tsd_mod.Context(gpu_ctx.device)
    uid = C.create_string_buffer(128)
    check(lib().tsd_dist_unique_id(uid))
    check(lib().tsd_dist_init(c.h, 0, 1, uid))
    n = C.c_int(0)
    check(lib().tsd_dist_comm_count(c.h, C.byref(n)))
    uid2 = C.create_string_buffer(128)
    check(lib().tsd_dist_unique_id(uid2))
    s0 = snap()
    assert lib().tsd_dist_init(c.h, 0, 1, uid2) == E.TSD_E_STATE, "a second tsd_dist_init overwrote the communicator"
    assert b"already holds a communicator" in lib().tsd_last_error()
    n2 = C.c_int(0)
    check(lib().tsd_dist_comm_count(c.h, C.byref(n2)))
    assert n.value == n2.value == 1 and moved(s0, snap()) == (0, 0)
    assert lib().tsd_ctx_destroy(c.h) == E.TSD_OK                # no tsd_dist_finalize: the destroy finalizes the communicator it holds
    c.h = None
    assert live(snap()) == live(a)
