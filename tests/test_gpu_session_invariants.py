"""GPU tests of the denoise session's step-invariant buffers (tsd_debug_set_session_hoist): the time path of every schedule entry and
the context K / V^T of all attention blocks are computed at upload() with the launches a step would make, so a session that reads
them gives the bits of one that recomputes them every step; nothing goes stale when parameters, the context or the schedule change;
the five launches are gone from the step; and a step allocates nothing."""
import numpy as np
import pytest

from oracle import rng

pytestmark = pytest.mark.gpu
SEED = 1234
N_TRAIN = 1000
SAMPLERS = [("ddpm", 0.0, "leading"), ("ddim", 0.5, "trailing"), ("dpmpp_2m", 0.0, "trailing")]
K_PROJ, T_PROJ = "unet.layer3.layer6.k_proj.weight", "unet.layer2.layer3.weight"


@pytest.fixture(scope="module")
def diffusion(gpu_ctx, tsd_mod):
    return tsd_mod.Diffusion(seed=SEED)


def _inputs(B, L, steps, T=77, tag=900):
    lat = rng.normal(SEED, tag, B * 4 * L * L).reshape(B, 4, L, L)
    ctx = rng.normal(SEED, tag + 1, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(SEED, tag + 2, B * T * 768).reshape(B, T, 768)
    noise = rng.normal(SEED, tag + 3, steps * B * 4 * L * L).reshape(steps, B, 4, L, L)
    return lat, ctx, uctx, noise


class hoist:
    """The context's switch for the sessions created inside; restored on exit (the context is shared by the whole run)."""

    def __init__(self, tsd_mod, gpu_ctx, on):
        self.lib, self.h, self.on = tsd_mod._lib.lib(), gpu_ctx.h, int(on)

    def __enter__(self):
        self.prev = self.lib.tsd_debug_set_session_hoist(self.h, self.on)
        assert self.prev in (0, 1)

    def __exit__(self, *exc):
        self.lib.tsd_debug_set_session_hoist(self.h, self.prev)


def _open(tsd_mod, model, B, L, sampler, cfg, steps, inputs, start=0):
    kind, eta, spacing = sampler
    lat, ctx, uctx, noise = inputs
    s = tsd_mod.Session(model, None, B, L, 77, cfg=cfg)
    s.set_sampler(kind, eta, spacing)
    s.set_schedule(N_TRAIN, steps, start)
    s.upload(lat, ctx, uctx if cfg else None, noise[start:], cfg_scale=7.5)
    return s


def _loop(tsd_mod, gpu_ctx, model, on, B, L, sampler, cfg, steps, order, inputs):
    """Latents after every step of `order`, from a session created and uploaded with the switch at `on`."""
    with hoist(tsd_mod, gpu_ctx, on):
        s = _open(tsd_mod, model, B, L, sampler, cfg, steps, inputs)
        assert s.hoist_info()["active"] == int(on)
        out = []
        for i in order:
            s.step(i)
            out.append(s.latents())
        s.close()
    return np.stack(out)


def _same(a, b, what):
    assert np.isfinite(a).all(), what
    for k in range(len(a)):
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k] - b[k]).max()))
    assert not np.array_equal(a[0], a[-1]), what   # the steps did something


# ---- 1. hoist on == hoist off, bitwise --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("B,L", [(2, 8), (3, 24)])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_hoisted_session_equals_the_per_step_session_bitwise(gpu_ctx, tsd_mod, diffusion, sampler, B, L, cfg):
    """Four steps, the last two out of order (2M then runs first order at step 3 and 2, on both sides alike)."""
    steps, order = 4, (0, 1, 3, 2)
    inputs = _inputs(B, L, steps, tag=900 + 10 * B)
    got = _loop(tsd_mod, gpu_ctx, diffusion.model, 1, B, L, sampler, cfg, steps, order, inputs)
    ref = _loop(tsd_mod, gpu_ctx, diffusion.model, 0, B, L, sampler, cfg, steps, order, inputs)
    _same(got, ref, (sampler[0], B, L, cfg))


def test_hoisted_session_equals_the_per_step_session_at_the_headline_shape(gpu_ctx, tsd_mod, diffusion):
    B, L, steps = 8, 64, 2
    inputs = _inputs(B, L, steps, tag=960)
    got = _loop(tsd_mod, gpu_ctx, diffusion.model, 1, B, L, SAMPLERS[0], False, steps, (0, 1), inputs)
    ref = _loop(tsd_mod, gpu_ctx, diffusion.model, 0, B, L, SAMPLERS[0], False, steps, (0, 1), inputs)
    _same(got, ref, "headline")


def test_hoisted_session_equals_the_per_step_session_full_size_unet(gpu_ctx, tsd_mod):
    full = tsd_mod.Diffusion(seed=SEED, variant="diffusion_sd15")
    try:
        B, L, steps = 2, 16, 3
        inputs = _inputs(B, L, steps, tag=970)
        for cfg in (False, True):
            got = _loop(tsd_mod, gpu_ctx, full.model, 1, B, L, SAMPLERS[2], cfg, steps, (0, 1, 2), inputs)
            ref = _loop(tsd_mod, gpu_ctx, full.model, 0, B, L, SAMPLERS[2], cfg, steps, (0, 1, 2), inputs)
            _same(got, ref, ("full-size", cfg))
    finally:
        full.model.close()


# ---- 2. no stale state ------------------------------------------------------------------------------------------------------------
def _param(model, name):
    for i, (n, shape, used, bound) in enumerate(model.specs):
        if n == name:
            assert used
            return i, shape, bound
    raise KeyError(name)


@pytest.mark.parametrize("cfg", [False, True])
def test_parameters_set_after_upload_reach_the_next_step(gpu_ctx, tsd_mod, cfg):
    """set_param of a k_proj weight and of a time-projection weight between upload() and step(): the step rebuilds the buffers (a
    rebuild, not an error) and gives the bits of a session created after the change - which differ from those of the old weights."""
    own = tsd_mod.Diffusion(seed=SEED)   # this test changes parameters: a model of its own
    try:
        B, L, steps = 2, 8, 3
        inputs = _inputs(B, L, steps, tag=980)
        with hoist(tsd_mod, gpu_ctx, 1):
            s = _open(tsd_mod, own.model, B, L, SAMPLERS[1], cfg, steps, inputs)
            s.step(0)
            before = s.latents()
            s.upload(*_upload_args(inputs, cfg))
            assert s.hoist_info()["builds"] == 2
            for k, name in enumerate((K_PROJ, T_PROJ)):
                i, shape, bound = _param(own.model, name)
                own.model.set_param(i, rng.uniform(SEED, 990 + k, int(np.prod(shape)), bound).reshape(shape))
            s.step(0)
            assert s.hoist_info()["builds"] == 3
            s.step(1)
            assert s.hoist_info()["builds"] == 3
            got = s.latents()
            s.close()
            fresh = _open(tsd_mod, own.model, B, L, SAMPLERS[1], cfg, steps, inputs)
            fresh.step(0)
            first = fresh.latents()
            fresh.step(1)
            ref = fresh.latents()
            fresh.close()
        assert np.isfinite(got).all() and np.array_equal(got, ref)
        assert not np.array_equal(first, before)   # the new weights change the result: a stale buffer would show
        ref_off = _loop(tsd_mod, gpu_ctx, own.model, 0, B, L, SAMPLERS[1], cfg, steps, (0, 1), inputs)
        assert np.array_equal(ref_off[1], got)
    finally:
        own.model.close()


def _upload_args(inputs, cfg, start=0):
    lat, ctx, uctx, noise = inputs
    return lat, ctx, uctx if cfg else None, noise[start:], 7.5


@pytest.mark.parametrize("cfg", [False, True])
def test_second_upload_with_another_context_is_a_fresh_session(gpu_ctx, tsd_mod, diffusion, cfg):
    B, L, steps = 2, 8, 3
    a, b = _inputs(B, L, steps, tag=1000), _inputs(B, L, steps, tag=1010)
    with hoist(tsd_mod, gpu_ctx, 1):
        s = _open(tsd_mod, diffusion.model, B, L, SAMPLERS[0], cfg, steps, a)
        s.step(0)
        first = s.latents()
        s.upload(*_upload_args(b, cfg))
        s.step(0)
        s.step(1)
        got = s.latents()
        s.close()
        fresh = _open(tsd_mod, diffusion.model, B, L, SAMPLERS[0], cfg, steps, b)
        fresh.step(0)
        other = fresh.latents()
        fresh.step(1)
        ref = fresh.latents()
        fresh.close()
    assert np.isfinite(got).all() and np.array_equal(got, ref)
    assert not np.array_equal(first, other)


def test_set_schedule_then_upload_uses_the_new_timesteps(gpu_ctx, tsd_mod, diffusion):
    """3 entries, then 5 (the table grows), then 2 entries from start_step 3 of 5: each equals the per-step session on that schedule."""
    B, L = 2, 8
    inputs = _inputs(B, L, 5, tag=1020)
    lat, ctx, uctx, noise = inputs
    with hoist(tsd_mod, gpu_ctx, 1):
        s = _open(tsd_mod, diffusion.model, B, L, SAMPLERS[1], False, 3, (lat, ctx, uctx, noise[:3]))
        ts3 = [s.timestep(i) for i in range(s.num_steps)]
        s.step(1)
        got = {}
        for n, start in ((5, 0), (5, 3)):
            s.set_schedule(N_TRAIN, n, start)
            assert [s.timestep(i) for i in range(s.num_steps)] != ts3
            with pytest.raises(tsd_mod.TsdError):
                s.step(0)                      # the upload is stale, as before
            s.upload(*_upload_args(inputs, False, start))
            out = []
            for i in range(s.num_steps):
                s.step(i)
                out.append(s.latents())
            got[(n, start)] = np.stack(out)
        s.close()
    with hoist(tsd_mod, gpu_ctx, 0):
        for (n, start), g in got.items():
            r = _open(tsd_mod, diffusion.model, B, L, SAMPLERS[1], False, n, inputs, start)
            assert r.num_steps == len(g) == n - start
            for i in range(r.num_steps):
                r.step(i)
                assert np.array_equal(r.latents(), g[i]), (n, start, i)
            r.close()


# ---- 3. the launches are gone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
def test_step_launches_neither_the_time_path_nor_the_context_projection(gpu_ctx, tsd_mod, diffusion, cfg):
    B, L, steps, P = 2, 8, 4, 3
    Bu, Tp, CK = (2 * B if cfg else B), 80, 6720
    inputs = _inputs(B, L, steps, tag=1030)

    def profile(on):
        with hoist(tsd_mod, gpu_ctx, on):
            s = _open(tsd_mod, diffusion.model, B, L, SAMPLERS[0], cfg, steps, inputs)
            s.step(0)                          # steady state: the profiled steps follow a step
            gpu_ctx.profile_begin()
            try:
                for i in range(1, 1 + P):
                    s.step(i)
                recs = gpu_ctx.profile_records()
            finally:
                prof = gpu_ctx.profile_end()
            s.close()
        total = sum(n for _, n in prof.values())
        assert total % P == 0
        small = [r for r in recs if r[0] == "small_linear"]
        kv = [r for r in recs if r[0] == "gemm" and r[1] == Bu * Tp and r[2] == 2 * CK]
        return total // P, len(small), len(kv)

    n_on, small_on, kv_on = profile(1)
    n_off, small_off, kv_off = profile(0)
    print(f"[hoist] cfg={cfg}: launches per step {n_off} -> {n_on}")
    assert (small_off, kv_off) == (3 * P, P)   # the per-step path has them: the records can tell
    assert (small_on, kv_on) == (0, 0)
    assert n_off - n_on == 5


# ---- 4. no allocation in a step ---------------------------------------------------------------------------------------------------
def test_steps_allocate_nothing(gpu_ctx, tsd_mod, diffusion):
    """No allocation counter exists: the buffers' addresses and their allocated bytes after 20 steps are those after upload(), and
    they were built once."""
    B, L, steps = 2, 8, 20
    inputs = _inputs(B, L, steps, tag=1040)
    with hoist(tsd_mod, gpu_ctx, 1):
        s = _open(tsd_mod, diffusion.model, B, L, SAMPLERS[0], True, steps, inputs)
        at_upload = s.hoist_info()
        assert at_upload["active"] == 1 and at_upload["builds"] == 1
        assert at_upload["time_table"] and at_upload["ctx_k"] and at_upload["ctx_vt"]
        assert at_upload["bytes"] >= 2 * (2 * B) * 80 * 6720 * 2 + steps * 6720 * 4
        s.step(0)
        after_one = s.hoist_info()
        for i in range(1, steps):
            s.step(i)
        assert np.isfinite(s.latents()).all()
        assert s.hoist_info() == after_one == at_upload
        s.close()
