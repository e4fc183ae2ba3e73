"""GPU: FreeU (csrc/kernels_freeu.hip, `tsd_model_set_freeu`) against tests/freeu_ref.py.

1. The launch alone, element-wise under the derived bound of freeu_ref (every element compared, none excluded), at six shapes from a 2 x 2
   plane to 64 x 64, on noise, constant planes (r' = s r), a cosine along y (r' = (1 + s) / 2 r for H > 2 - half of a cosine's energy sits
   in bin +1, which the mask does not hold - and s r at H = 2, where bin -1 is the Nyquist bin) and a checkerboard (r' = r); s in
   {0.9, 0.2, -0.5}, b in {1.5, 0.5}, both modes; the identity paths, guard bands and pitch gaps, bits run to run, across batch positions
   and under the jitter build.
2. The model: kinds 6 and 16 at latents 16 x 16 and 16 x 32, both conventions and both modes against `diffusion_freeu`, a table that
   only touches the levels whose producers emit GroupNorm statistics, ControlNet + FreeU, the all-ones table, the launch counts.
3. Sessions: bitwise the host-driven loop, switching inside an open session, slots against lockstep, generate(freeu=...).
4. Refusals.

Run as `python tests/test_gpu_freeu.py jitter-child REPEATS` this file is the child of the jitter test: it prints one JSON line of digests
per case on whatever library TSD_LIB names."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "stable-diffusion.mojo_amd"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import pytest

import freeu_ref as F
from oracle import rng
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, rel_l2

pytestmark = pytest.mark.gpu
JITTER_REPEATS = 8
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")

# ---- 1. the launch ------------------------------------------------------------------------------------------------------------------------
# (B, H, W, Ch, Cr): the 2 x 2 plane with fewer channels than a chunk, a channel count that is no multiple of the chunk (24), the bottleneck
# and two decoder levels, more than one pixel slab (6 x 10 = 60 < 256 < 16 x 16 < 64 x 64) and the largest plane of the issue
SHAPES = ((2, 2, 2, 16, 8), (3, 2, 4, 64, 24), (2, 4, 4, 1280, 640), (2, 6, 10, 640, 320), (1, 16, 16, 1280, 1280), (1, 64, 64, 320, 320))
FAMILIES = ("noise", "constant", "cosine", "checker")
# every s and every (b, mode) in four launches
COMBOS = ((0.9, 1.5, F.CONSTANT), (0.2, 0.5, F.CONSTANT), (-0.5, 1.5, F.MODULATED), (0.9, 0.5, F.MODULATED))


def _skip_input(family, shape, seed):
    B, H, W, _, Cr = shape
    g = np.random.default_rng(seed)
    if family == "noise":
        return g.normal(size=(B, H, W, Cr)).astype(np.float16)
    amp = g.normal(size=(B, 1, 1, Cr))
    y, x = np.arange(H).reshape(1, H, 1, 1), np.arange(W).reshape(1, 1, W, 1)
    if family == "constant":
        plane = np.ones((1, H, W, 1))
    elif family == "cosine":
        plane = np.cos(2 * np.pi * y / H) * np.ones((1, 1, W, 1))
    else:
        plane = np.where((y + x) % 2 == 0, 1.0, -1.0)
    return (amp * plane).astype(np.float16)


def _hidden_input(shape, seed, mode):
    """Noise; in the modulated mode plus a per-pixel ramp over [0, 1], so that hi - lo is O(1)."""
    B, H, W, Ch, _ = shape
    h = np.random.default_rng(seed).normal(size=(B, H, W, Ch))
    if mode == F.MODULATED:
        h = h + np.linspace(0.0, 1.0, H * W).reshape(1, H, W, 1)
    return h.astype(np.float16)


_WORST = {}


def _hold(name, got, want, bound):
    ratio = np.abs(got.astype(np.float64) - want) / np.where(bound > 0, bound, 1.0)
    exact = bound == 0
    assert np.array_equal(got.astype(np.float64)[exact], want[exact]), f"{name}: an element with bound 0 moved"
    worst = float(ratio[~exact].max()) if (~exact).any() else 0.0
    _WORST[name.split()[0]] = max(_WORST.get(name.split()[0], 0.0), worst)
    assert worst <= 1.0, f"{name}: worst error / bound {worst:.3f} at {np.unravel_index(np.argmax(np.where(exact, 0, ratio)), ratio.shape)}"
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_launch_is_under_the_derived_bound_elementwise(gpu_ctx, tsd_mod, shape):
    for fi, family in enumerate(FAMILIES):
        if family == "checker" and min(shape[1], shape[2]) < 4:
            continue
        r = _skip_input(family, shape, 100 + fi)
        for s, b, mode in COMBOS:
            h = _hidden_input(shape, 200 + fi, mode) if family == "noise" else None   # the hidden half does not depend on the skip's family
            ho, ro = tsd_mod.freeu(h, r, b, s, mode)
            want, bound = F.skip_bound(r, s)
            w = _hold(f"skip/{family} {shape} s={s}", ro, want, bound)
            r64 = r.astype(np.float64)
            if family == "constant":       # P = r: the whole plane is bin (0, 0) (a constant stays one when rounded to fp16)
                assert np.abs(want - s * r64).max() <= 1e-12
            elif family == "cosine":       # half of it is bin fy = -1 - all of it at H = 2.  The fp16 plane is the cosine plus a rounding
                # d, |d| <= 2^-11 max|r|; the filter is linear with |P(d)| <= 7 max|d|, so the plane misses c r by (1 + 7 |s - 1| + |c|) max|d|
                c = s if shape[1] == 2 else 0.5 * (1 + s)
                assert np.abs(want - c * r64).max() <= (1 + 7 * abs(s - 1) + abs(c)) * 2.0 ** -11 * np.abs(r64).max()
            elif family == "checker":      # all of it is the Nyquist bin of both axes: P = 0 (+-a stays +-a when rounded)
                assert np.abs(want - r64).max() <= 1e-12
            if h is not None:
                want, bound = F.hidden_bound(h, b, mode)
                wh = _hold(f"hidden/{'modulated' if mode else 'constant'} {shape} b={b}", ho, want, bound)
                assert np.array_equal(ho[..., shape[3] // 2:].view(np.uint16), h[..., shape[3] // 2:].view(np.uint16))
                print(f"[freeu] {shape} {family} s={s} b={b} mode={mode}: worst error / bound skip {w:.3f} hidden {wh:.3f}")
    print("[freeu] worst error / bound per family so far: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(_WORST.items())))


def test_modulated_mode_with_a_constant_mean_leaves_the_hidden_tensor_alone(gpu_ctx, tsd_mod):
    """hi == lo: every pixel holds the same channel vector, the device's means are one fp32 value, n = 0 and h comes back bit for bit (the
    published code divides by zero here)."""
    B, H, W, Ch, Cr = 2, 6, 10, 640, 320
    row = np.random.default_rng(7).normal(size=(B, 1, 1, Ch)).astype(np.float16)
    h = np.ascontiguousarray(np.broadcast_to(row, (B, H, W, Ch)))
    ho, _ = tsd_mod.freeu(h, None, 1.5, 1.0, F.MODULATED)
    assert np.isfinite(ho.astype(np.float32)).all()
    assert np.array_equal(ho.view(np.uint16), h.view(np.uint16))
    assert np.array_equal(F.hidden_modulated(h, 1.5), h.astype(np.float64))


def _guarded(tsd_mod, gpu_ctx, h, r, ldh, ldr, guard, b, s, mode):
    """tsd_debug_freeu_run on [guard | B H W ld | guard] buffers filled with a pattern outside the tensors -> the buffers as they came back."""
    B, H, W, Ch = h.shape
    Cr = r.shape[3]

    def embed(x, ld):
        rows = np.full((B * H * W, ld), 0x7BCD, np.uint16)   # a finite fp16 pattern
        rows[:, : x.shape[3]] = x.reshape(-1, x.shape[3]).view(np.uint16)
        return np.concatenate([np.full(guard, 0x5A5A, np.uint16), rows.reshape(-1), np.full(guard, 0x5A5A, np.uint16)])
    hb, rb = embed(h, ldh), embed(r, ldr)
    ho, ro = np.empty_like(hb), np.empty_like(rb)
    tsd_mod._lib.check(tsd_mod._lib.lib().tsd_debug_freeu_run(gpu_ctx.h, hb.ctypes.data, rb.ctypes.data, B, H, W, Ch, Cr, ldh, ldr, guard, float(b),
                                                              float(s), int(mode), ho.ctypes.data, ro.ctypes.data))
    return hb, rb, ho, ro


@pytest.mark.parametrize("shape", (SHAPES[1], SHAPES[3]), ids=lambda s: "x".join(map(str, s)))
def test_identity_paths_guard_bands_and_pitch_gaps(gpu_ctx, tsd_mod, shape):
    B, H, W, Ch, Cr = shape
    h, r = _hidden_input(shape, 31, F.MODULATED), _skip_input("noise", shape, 32)
    bits = lambda a: a.view(np.uint16)
    # s = 1: r bit for bit; b = 1: h bit for bit; both: nothing is launched at all
    for mode in (F.CONSTANT, F.MODULATED):
        ho, ro = tsd_mod.freeu(h, r, 1.5, 1.0, mode)
        assert np.array_equal(bits(ro), bits(r)) and not np.array_equal(bits(ho), bits(h))
        ho, ro = tsd_mod.freeu(h, r, 1.0, 0.2, mode)
        assert np.array_equal(bits(ho), bits(h)) and not np.array_equal(bits(ro), bits(r))
        ho, ro = tsd_mod.freeu(h, r, 1.0, 1.0, mode)
        assert np.array_equal(bits(ho), bits(h)) and np.array_equal(bits(ro), bits(r))
    # pitches wider than the tensors and guard bands on both sides: only columns < Ch / 2 of h and < Cr of r may change
    ldh, ldr, guard = Ch + 24, Cr + 8, 64
    for mode in (F.CONSTANT, F.MODULATED):
        hb, rb, ho, ro = _guarded(tsd_mod, gpu_ctx, h, r, ldh, ldr, guard, 1.5, 0.2, mode)
        dense_h, dense_r = tsd_mod.freeu(h, r, 1.5, 0.2, mode)
        rows_h, rows_r = ho[guard:-guard].reshape(-1, ldh), ro[guard:-guard].reshape(-1, ldr)
        assert np.array_equal(ho[:guard], hb[:guard]) and np.array_equal(ho[-guard:], hb[-guard:])
        assert np.array_equal(ro[:guard], rb[:guard]) and np.array_equal(ro[-guard:], rb[-guard:])
        assert np.array_equal(rows_h[:, Ch // 2:], hb[guard:-guard].reshape(-1, ldh)[:, Ch // 2:])     # the upper half and the gap
        assert np.array_equal(rows_r[:, Cr:], rb[guard:-guard].reshape(-1, ldr)[:, Cr:])
        # and the pitch does not change a bit of the result
        assert np.array_equal(rows_h[:, :Ch], bits(dense_h).reshape(-1, Ch)) and np.array_equal(rows_r[:, :Cr], bits(dense_r).reshape(-1, Cr))


def _digest(arrays):
    d = hashlib.sha1()
    for a in arrays:
        d.update(np.ascontiguousarray(a).tobytes())
    return d.hexdigest()


def bitwise_cases(tsd_mod, repeats):
    """[(name, [digest per repeat])] of the launch at three shapes, both modes."""
    out = []
    for shape in (SHAPES[1], SHAPES[3], SHAPES[4]):
        for mode in (F.CONSTANT, F.MODULATED):
            h, r = _hidden_input(shape, 41, F.MODULATED), _skip_input("noise", shape, 42)
            out.append((f"{shape} mode {mode}", [_digest(tsd_mod.freeu(h, r, 1.5, 0.2, mode)) for _ in range(repeats)]))
    return out


def test_bits_do_not_depend_on_the_run_the_batch_or_the_batch_position(gpu_ctx, tsd_mod):
    for name, digests in bitwise_cases(tsd_mod, 3):
        assert len(set(digests)) == 1, f"{name}: {len(set(digests))} results in 3 runs"
    shape = (3, 6, 10, 640, 320)
    for mode in (F.CONSTANT, F.MODULATED):
        h, r = _hidden_input(shape, 51, F.MODULATED), _skip_input("noise", shape, 52)
        ho, ro = tsd_mod.freeu(h, r, 1.5, 0.2, mode)
        for k in range(3):   # sample k of B = 3 equals the same sample alone
            h1, r1 = tsd_mod.freeu(h[k:k + 1], r[k:k + 1], 1.5, 0.2, mode)
            assert np.array_equal(h1[0].view(np.uint16), ho[k].view(np.uint16)) and np.array_equal(r1[0].view(np.uint16), ro[k].view(np.uint16)), (mode, k)
        # ... and does not depend on how many channels sit beside it
        _, r_half = tsd_mod.freeu(None, np.ascontiguousarray(r[..., :160]), 1.0, 0.2, mode)
        assert np.array_equal(r_half.view(np.uint16), np.ascontiguousarray(ro[..., :160]).view(np.uint16))


def test_jitter_build_reproduces_the_shipped_bits(tsd_mod, gpu_ctx):
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    here = bitwise_cases(tsd_mod, 1)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [t["name"] for t in there] == [n for n, _ in here]
    for (name, mine), theirs in zip(here, there):
        assert len(theirs["digests"]) == JITTER_REPEATS
        assert all(dg == mine[0] for dg in theirs["digests"]), f"{name}: the jitter build gave {len(set(theirs['digests']))} result(s), not the shipped bits"


# ---- 2. the model -------------------------------------------------------------------------------------------------------------------------
# a table that only touches the 8 x 8 and 16 x 16 levels of a 16 x 16 latent (64 and 256 pixels): the levels whose producers emit GroupNorm
# statistics (one slab per 32 rows; act_alloc_gn / gn_emit) - a rewritten tensor that kept them would normalise with stale statistics
LATE_TABLE = (np.array([1.0] * 6 + [1.6] * 6, np.float32), np.array([1.0] * 6 + [0.4] * 6, np.float32))
CONFIGS = [(conv, mode) for conv in ("diffusers", "channels") for mode in (F.CONSTANT, F.MODULATED)]


class World:
    """One kind's model with numpy-drawn parameters, built once per module; references are computed once per case and kept."""

    def __init__(self, tsd_mod, kind):
        from controlnet_ref import draw_params
        self.kind, self.tsd = kind, tsd_mod
        self.P = draw_params(tsd_mod.param_specs(kind), F.MODEL_SEED)
        self.d = tsd_mod.Diffusion(params=self.P, variant=kind)
        self.steps = F.model_steps(kind)
        self._ref, self._plain = {}, {}

    def inputs(self, shape):
        return F.model_inputs(self.kind, *shape)

    def reference(self, shape, table, mode, key):
        if (shape, key, mode) not in self._ref:
            lat, ctx, temb = self.inputs(shape)
            self._ref[(shape, key, mode)] = F.diffusion_freeu(self.P, lat[0], ctx[0], temb[0], table, mode, steps=self.steps, tn=True)[None]
        return self._ref[(shape, key, mode)]

    def plain(self, shape):
        if shape not in self._plain:
            assert self.d.freeu is None
            self._plain[shape] = self.d.forward(*self.inputs(shape))
        return self._plain[shape]

    def close(self):
        self.d.model.close()


_WORLDS = {}


def _world(tsd_mod, kind):
    if kind not in _WORLDS:
        _WORLDS[kind] = World(tsd_mod, kind)
    return _WORLDS[kind]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _WORLDS.values():
        w.close()
    _WORLDS.clear()


@pytest.fixture(scope="module", params=list(F.MODEL_KINDS))
def world(request, gpu_ctx, tsd_mod):
    return _world(tsd_mod, request.param)


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{'modulated' if c[1] else 'constant'}")
@pytest.mark.parametrize("shape", F.MODEL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_with_freeu_matches_the_reference(world, tsd_mod, shape, config):
    conv, mode = config
    table = tsd_mod.freeu_table(convention=conv, **F.MODEL_VALUES)
    ref = world.reference(shape, table, mode, conv)
    plain = world.plain(shape)
    world.d.set_freeu(convention=conv, modulated=bool(mode), **F.MODEL_VALUES)
    try:
        b, s, m = world.d.freeu
        assert np.array_equal(b, table[0]) and np.array_equal(s, table[1]) and m == mode
        out = world.d.forward(*world.inputs(shape))
        again = world.d.forward(*world.inputs(shape))
    finally:
        world.d.clear_freeu()
    assert world.d.freeu is None
    assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, f"{world.kind} {shape} {conv} mode {mode}")
    acts = rel_l2(out, plain)
    print(f"[freeu] {world.kind} {shape} {conv} mode {mode}: rel_l2 against the plain forward {acts:.3e}")
    assert acts > 10 * TOL_MODEL
    np.testing.assert_array_equal(out, again)
    np.testing.assert_array_equal(world.d.forward(*world.inputs(shape)), plain)     # cleared: the plain bits are back


def test_stale_statistics_would_show_at_the_levels_whose_producers_emit_them(world, tsd_mod):
    shape = F.MODEL_SHAPES[0]
    for mode in (F.CONSTANT, F.MODULATED):
        ref = world.reference(shape, LATE_TABLE, mode, "late")
        world.d.set_freeu(table=LATE_TABLE, modulated=bool(mode))
        try:
            out = world.d.forward(*world.inputs(shape))
        finally:
            world.d.clear_freeu()
        assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, f"{world.kind} {shape} late table mode {mode}")
        assert rel_l2(out, world.plain(shape)) > 10 * TOL_MODEL


def test_all_ones_is_the_plain_forward_and_the_launch_counts(world, tsd_mod, gpu_ctx):
    shape = F.MODEL_SHAPES[0]
    plain = world.plain(shape)
    ones = (np.ones(12, np.float32), np.ones(12, np.float32))

    def counted():
        gpu_ctx.profile_begin()
        out = world.d.forward(*world.inputs(shape))
        return out, {k: v[1] for k, v in gpu_ctx.profile_end().items()}
    base_out, base = counted()
    np.testing.assert_array_equal(base_out, plain)
    world.d.set_freeu(table=ones, modulated=True)
    try:
        assert world.d.freeu is None          # a table of all ones is off
        out, n = counted()
    finally:
        world.d.clear_freeu()
    np.testing.assert_array_equal(out, plain)
    assert n == base, (n, base)
    for mode, per_block in ((F.CONSTANT, 1), (F.MODULATED, 2)):
        world.d.set_freeu(convention="diffusers", modulated=bool(mode), **F.MODEL_VALUES)
        try:
            _, n = counted()
        finally:
            world.d.clear_freeu()
        assert n["elementwise"] - base["elementwise"] == 6 * per_block, (mode, n, base)
        assert all(n[k] == base[k] for k in n if k not in ("elementwise", "groupnorm")), (n, base)


def test_controlnet_and_freeu_compose(tsd_mod, gpu_ctx):
    """Kind 6 with a ControlNet at scale 0.5 and FreeU (channels convention): the injection runs first, as in diffusers."""
    import controlnet_ref as R
    from oracle import ops
    w = _world(tsd_mod, "diffusion_sd15_torch")
    PC = R.draw_params(tsd_mod.param_specs("controlnet_sd15_torch"), 5, nonzero=("zero.", "hint.conv8"))
    cn = tsd_mod.ControlNet(params=PC, variant="controlnet_sd15_torch")
    try:
        shape = F.MODEL_SHAPES[0]
        lat, ctx, temb = w.inputs(shape)
        hint = (rng.uniform(7, 802, 3 * 64 * shape[0] * shape[1], 0.5) + np.float32(0.5)).reshape(1, 3, 8 * shape[0], 8 * shape[1])
        table = tsd_mod.freeu_table(convention="channels", **F.MODEL_VALUES)
        res = R.controlnet(PC, lat[0], ctx[0], temb[0], hint[0], tn=True)
        ref = F.diffusion_freeu(w.P, lat[0], ctx[0], temb[0], table, F.CONSTANT, tn=True, res=res, res_scale=0.5)[None]
        only_control = w.d.forward(lat, ctx, temb, control=cn, hint=hint, control_scale=0.5)
        w.d.set_freeu(table=table)
        out = w.d.forward(lat, ctx, temb, control=cn, hint=hint, control_scale=0.5)
        only_freeu = w.d.forward(lat, ctx, temb)
        assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, "ControlNet + FreeU")
        assert rel_l2(out, only_control) > 10 * TOL_MODEL and rel_l2(out, only_freeu) > 1e-2
    finally:
        w.d.clear_freeu()
        cn.model.close()


# ---- 3. sessions --------------------------------------------------------------------------------------------------------------------------
import test_gpu_controlnet as TC   # the host-driven loop and the session driver of the control tests: FreeU is state of the model they drive

S_TABLE_KW = dict(convention="channels", **F.MODEL_VALUES)
S_CASES = [c for c in TC.S_CASES if c[0] in ("ddpm_seeded", "dpmpp_2m")]


@pytest.fixture(scope="module")
def unet(gpu_ctx, tsd_mod):
    d = tsd_mod.Diffusion(seed=TC.SEED, variant="diffusion_sd15")
    yield d
    d.model.close()


@pytest.mark.parametrize("on", [1, 0], ids=["hoist", "nohoist"])
@pytest.mark.parametrize("case", S_CASES, ids=[c[0] for c in S_CASES])
def test_cfg_session_with_freeu_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, unet, case, on):
    inputs = TC._s_inputs(1900)
    with TC.hoist(tsd_mod, gpu_ctx, on):
        plain = TC.session_run(tsd_mod, unet, None, case, True, inputs, None)
        unet.set_freeu(**S_TABLE_KW)
        try:
            got = TC.session_run(tsd_mod, unet, None, case, True, inputs, None)
            want = TC.host_loop(tsd_mod, gpu_ctx, unet, None, case, True, inputs, lambda i: None)
        finally:
            unet.clear_freeu()
    for i in range(TC.S_STEPS):
        assert np.isfinite(got[i]).all()
        assert TC._same(got[i], want[i]), (case[0], on, i, float(np.abs(got[i] - want[i]).max()))
    assert rel_l2(got[-1], plain[-1]) > 1e-3


@pytest.mark.parametrize("modulated", [False, True], ids=["constant", "modulated"])
def test_setting_and_clearing_inside_an_open_session_acts_on_the_next_step(gpu_ctx, tsd_mod, unet, modulated):
    case, inputs = TC.S_CASES[0], TC._s_inputs(1910)
    lat, ctx, uctx, _, _ = inputs
    s = TC._open(tsd_mod, unet, True, case[1], case[2], case[3])
    s.upload(lat, ctx, uctx, None, cfg_scale=TC.S_CFG_SCALE)
    s.set_seeds(TC.S_SEEDS)
    got = []
    try:
        s.step(0); got.append(s.latents())
        unet.set_freeu(modulated=modulated, **S_TABLE_KW)
        s.step(1); got.append(s.latents())
        unet.clear_freeu()
        s.step(2); got.append(s.latents())
    finally:
        unet.clear_freeu()
        s.close()
    loop = lambda x0, first: TC.host_loop(tsd_mod, gpu_ctx, unet, None, case, True, inputs, lambda i: None, x0=x0, first=first, steps=first + 1)[0]
    w0 = loop(None, 0)
    unet.set_freeu(modulated=modulated, **S_TABLE_KW)
    try:
        w1 = loop(w0, 1)
    finally:
        unet.clear_freeu()
    w2 = loop(w1, 2)
    w1_plain = loop(w0, 1)
    assert TC._same(got[0], w0) and TC._same(got[1], w1) and TC._same(got[2], w2)
    assert not TC._same(w1, w1_plain)


def test_slot_session_equals_the_lockstep_one_bitwise(gpu_ctx, tsd_mod, unet):
    B, L, T, steps = 2, TC.S_L, TC.T, TC.S_STEPS
    ctx = rng.normal(7, 1920, B * T * 768).reshape(B, T, 768)
    uctx = rng.normal(7, 1921, B * T * 768).reshape(B, T, 768)
    seeds = [4242, 777]
    unet.set_freeu(modulated=True, **S_TABLE_KW)
    try:
        lock = tsd_mod.Session(unet.model, None, B, L, T, cfg=True)
        lock.set_schedule(TC.S_NTRAIN, steps, 0)
        lock.upload(np.zeros((B, 4, L, L), np.float32), ctx, uctx, None, cfg_scale=TC.S_CFG_SCALE)
        lock.set_seeds(seeds)
        lock.seed_latents()
        for i in range(steps):
            lock.step(i)
        want = lock.latents()
        lock.close()
        slots = tsd_mod.Session(unet.model, None, B, L, T, cfg=True)
        slots.set_schedule(TC.S_NTRAIN, steps, 0)
        slots.slots_open()
        for k in range(B):
            slots.slot_start(k, ctx[k], uctx[k], seed=seeds[k], cfg_scale=TC.S_CFG_SCALE)
        for _ in range(steps):
            slots.advance()
        got = np.stack([slots.slot_latents(k) for k in range(B)])
        slots.close()
    finally:
        unet.clear_freeu()
    assert np.isfinite(got).all() and TC._same(got, want)
    plain = tsd_mod.Session(unet.model, None, B, L, T, cfg=True)
    plain.set_schedule(TC.S_NTRAIN, steps, 0)
    plain.upload(np.zeros((B, 4, L, L), np.float32), ctx, uctx, None, cfg_scale=TC.S_CFG_SCALE)
    plain.set_seeds(seeds)
    plain.seed_latents()
    for i in range(steps):
        plain.step(i)
    assert not TC._same(plain.latents(), want)
    plain.close()


def test_generate_with_freeu_is_the_explicit_session_and_restores_the_table(gpu_ctx, tsd_mod, unet):
    lat, ctx, uctx, _, _ = TC._s_inputs(1930)
    kw = dict(uncond_context=uctx, cfg=True, cfg_scale=TC.S_CFG_SCALE, inference_steps=3, strength=1.0, L=TC.S_L, return_latents=True, seeds=TC.S_SEEDS)
    mine = tsd_mod.freeu_table(1.2, 1.3, 0.8, 0.7)
    unet.set_freeu(table=mine, modulated=True)      # what the model held before the call
    try:
        out = tsd_mod.generate(unet, None, ctx, freeu=dict(S_TABLE_KW), **kw)
        b, s, mode = unet.freeu
        assert np.array_equal(b, mine[0]) and np.array_equal(s, mine[1]) and mode == F.MODULATED
        with pytest.raises(ValueError):             # a refused argument inside the call: the table is back as well
            tsd_mod.generate(unet, None, ctx, freeu=dict(S_TABLE_KW), controlnet=object(), **kw)
        assert np.array_equal(unet.freeu[0], mine[0]) and unet.freeu[2] == F.MODULATED
        unet.clear_freeu()
        plain = tsd_mod.generate(unet, None, ctx, **kw)
        assert unet.freeu is None
        again = tsd_mod.generate(unet, None, ctx, freeu=dict(S_TABLE_KW), **kw)
        assert unet.freeu is None
        unet.set_freeu(**S_TABLE_KW)
        s = tsd_mod.Session(unet.model, None, TC.S_B, TC.S_L, TC.T, cfg=True)
        s.set_schedule(TC.S_NTRAIN, 3, 0)
        s.upload(np.zeros_like(lat), ctx, uctx, None, cfg_scale=TC.S_CFG_SCALE)
        s.set_seeds(TC.S_SEEDS)
        s.seed_latents()
        for i in range(3):
            s.step(i)
        want = s.latents()
        s.close()
    finally:
        unet.clear_freeu()
    assert TC._same(out, want) and TC._same(again, want) and not TC._same(out, plain)
    stream = list(tsd_mod.generate_stream(unet, None, [tsd_mod.Request(0, ctx[0], uctx[0], seed=TC.S_SEEDS[0], cfg_scale=TC.S_CFG_SCALE)], 1, TC.S_L,
                                          inference_steps=3, freeu=dict(S_TABLE_KW)))
    assert unet.freeu is None and len(stream) == 1 and TC._same(stream[0][1], want[0])


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx, tsd_mod, unet):
    E = tsd_mod._lib
    lib = E.lib()
    ones = np.ones(12, np.float32)
    good_b, good_s = tsd_mod.freeu_table(1.5, 1.6, 0.9, 0.2)
    others = [tsd_mod.Diffusion(seed=1), tsd_mod.Decoder(seed=1), tsd_mod.ControlNet(seed=1), tsd_mod.IPAdapter(seed=1)]
    try:
        for o in others:                            # the Tiny-SD graph, a VAE, a ControlNet, an adapter
            assert lib.tsd_model_set_freeu(o.model.h, E.ptr(good_b), E.ptr(good_s), 0) == E.TSD_E_ARG, o
            assert lib.tsd_model_freeu(o.model.h, None, None, None) == E.TSD_E_ARG
        with pytest.raises(tsd_mod.TsdError) as e:
            others[0].set_freeu(1.5, 1.6, 0.9, 0.2)
        assert e.value.code == E.TSD_E_ARG
    finally:
        for o in others:
            o.model.close()
    unet.set_freeu(table=(good_b, good_s))
    try:
        for bad in (np.nan, np.inf, -np.inf):       # a non-finite b or s
            for which in (0, 1):
                tab = [good_b.copy(), good_s.copy()]
                tab[which][7] = bad
                assert lib.tsd_model_set_freeu(unet.model.h, E.ptr(tab[0]), E.ptr(tab[1]), 0) == E.TSD_E_ARG
        for mode in (-1, 2):                        # a bad mode
            assert lib.tsd_model_set_freeu(unet.model.h, E.ptr(good_b), E.ptr(good_s), mode) == E.TSD_E_ARG
        assert lib.tsd_model_set_freeu(unet.model.h, E.ptr(good_b), None, 0) == E.TSD_E_ARG      # exactly one of b, s NULL
        assert lib.tsd_model_set_freeu(unet.model.h, None, E.ptr(good_s), 0) == E.TSD_E_ARG
        b, s, mode = unet.freeu                     # every refusal left the table as it was
        assert np.array_equal(b, good_b) and np.array_equal(s, good_s) and mode == 0
        assert lib.tsd_model_set_freeu(unet.model.h, None, None, 0) == 0 and unet.freeu is None
        assert lib.tsd_model_set_freeu(unet.model.h, E.ptr(ones), E.ptr(ones), 1) == 0 and unet.freeu is None
    finally:
        unet.clear_freeu()
    h, r = np.zeros((1, 4, 4, 32), np.float16), np.zeros((1, 4, 4, 16), np.float16)
    for kw, code in ((dict(b=np.nan), E.TSD_E_ARG), (dict(s=np.inf), E.TSD_E_ARG), (dict(mode=2), E.TSD_E_ARG)):
        with pytest.raises(tsd_mod.TsdError) as e:
            tsd_mod.freeu(h, r, **dict(dict(b=1.5, s=0.5, mode=0), **kw))
        assert e.value.code == code
    for hh, rr in ((np.zeros((1, 4, 4, 24), np.float16), r), (h, np.zeros((1, 4, 4, 12), np.float16)), (np.zeros((1, 1, 4, 32), np.float16), np.zeros((1, 1, 4, 16), np.float16))):
        with pytest.raises(tsd_mod.TsdError) as e:  # Ch % 16, Cr % 8, a one-row plane
            tsd_mod.freeu(hh, rr, 1.5, 0.5)
        assert e.value.code == E.TSD_E_SHAPE


def test_device_ledger_stays_balanced_and_the_tables_go_with_the_context(gpu_ctx, tsd_mod):
    before = tsd_mod.device_ledger()
    ctx2 = tsd_mod.Context(gpu_ctx.device)
    for H, W in ((2, 2), (4, 6), (8, 8)):           # three plane sizes: three context-held tables
        r = np.ones((1, H, W, 8), np.float16)
        tsd_mod.freeu(None, r, 1.0, 0.5, ctx=ctx2)
        tsd_mod.freeu(None, r, 1.0, 0.5, ctx=ctx2)  # the second call finds its table
    held = tsd_mod.device_ledger()
    ctx2.close()
    after = tsd_mod.device_ledger()
    assert held["ALLOCS_LIVE"] >= before["ALLOCS_LIVE"] + 3
    for k in ("ALLOCS_LIVE", "BYTES_LIVE", "EVENTS_LIVE", "STREAMS_LIVE", "CTX_LIVE", "FREES_UNKNOWN", "RELEASE_ERRORS"):
        assert after[k] == before[k], (k, before, held, after)


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    import tsd
    tsd.set_strict(True)
    for _name, _digests in bitwise_cases(tsd, int(sys.argv[2])):
        print(json.dumps({"name": _name, "digests": _digests}), flush=True)
