"""Windowed self attention (flash_attn_win_kernel) through version-3 descriptors of tsd_debug_attn_run, held to the plain launch of the
same instantiation on window-major gathered operands and to the plain kernels' fp64 bound; and the window table of a kind-6 model."""
import functools

import numpy as np
import pytest

import attn64_ref as R
import attn_ref as A
import freeu_ref as F                  # the numpy forward of the full-size UNets and the draw the model-level tests share
import replay
import test_gpu_controlnet as TC       # the host-driven loop and the session driver: the window table is state of the model they drive
from controlnet_ref import draw_params
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, rel_l2

pytestmark = pytest.mark.gpu
#        d, win, (gh, gw), B, H, kind
CASES = [(40, 8, (16, 24), 2, 8, "flat"), (40, 16, (32, 16), 1, 8, "flat"), (40, 32, (32, 64), 1, 8, "flat"), (64, 8, (16, 16), 1, 5, "flat"),
         (80, 16, (16, 32), 2, 2, "flat"), (160, 8, (8, 16), 1, 8, "flat"), (40, 64, (64, 128), 1, 1, "flat"),
         (40, 16, (16, 32), 1, 2, "rising"), (64, 16, (16, 32), 1, 2, "rising"), (80, 16, (16, 32), 1, 2, "rising"),
         (160, 16, (16, 32), 1, 2, "rising")]     # rising: 0 .. 40 log2 units along a window's 256 keys - its workgroups repeat exactly
IDS = [f"d{c[0]}-w{c[1]}-{c[2][0]}x{c[2][1]}-{c[5]}" for c in CASES]
KIND, WIN = "diffusion_sd15_torch", (8, 0, 0, 0)


def win_index(win, gh, gw):
    """[window][window-local index] -> token of the row-major gh x gw grid."""
    wy, wx = np.divmod(np.arange((gh // win) * (gw // win)), gw // win)
    i = np.arange(win * win)
    return (wy[:, None] * win + i[None] // win) * gw + wx[:, None] * win + i[None] % win


def to_grid(y, idx, B):
    n, m = idx.shape
    out = np.empty((B, y.shape[1], n * m, y.shape[3]), y.dtype)
    out[:, :, idx] = y.reshape(B, n, y.shape[1], m, y.shape[3]).transpose(0, 2, 1, 3, 4)
    return out


@functools.lru_cache(maxsize=None)
def case(i):
    """(windowed descriptor, its operands, gathered descriptor, its operands, window index) - built once, shared, never modified."""
    hd, win, (gh, gw), B, H, kind = CASES[i]
    idx = win_index(win, gh, gw)
    g = A.attn_desc(B * idx.shape[0], H, hd, win * win, win * win)
    g[A.AD["VERSION"]] = 2
    gops = (R if hd == 64 else A).make_inputs(g, kind, seed=11)
    d = A.attn_desc(B, H, hd, gh * gw, gh * gw)
    d[A.AD["VERSION"]] = 3
    d = np.concatenate([d, np.array([win, gh, gw], np.int64)])     # TSD_AD3_WIN, _GRID_H, _GRID_W
    return d, A.pack(d, *(to_grid(x, idx, B) for x in A.unpack_inputs(g, gops)[:3])), g, gops, idx


def run(ctx, d, ops):
    rc, outs, info = replay.run("tsd_debug_attn_run", ctx, d, ops, A.AO, A.INPUTS, ("O",), A.dtype_of, A.extents)
    assert rc == 0, replay.lib().tsd_last_error().decode()
    return outs["O"], {k: int(info[v]) for k, v in A.AI.items() if k != "COUNT"}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_windowed_launch_has_the_plain_launch_bits_and_is_inside_the_fp64_bound(gpu_ctx, i):
    (hd, win, _, B, _, kind), (d, ops, g, gops, idx) = CASES[i], case(i)
    out, info = run(gpu_ctx, d, ops)
    assert info["CHANGED"] == 0 and info["DIAG"] == 1
    replay.assert_gaps_hold_fill(out, A.o_index(d), "O")
    assert (hd, win) != (40, 32) or info["KERNEL"] == A.AK["40_2"]      # 1024 keys, 4 query tiles x 2 windows x 8 heads
    g = g.copy()
    if hd == 40:
        g[A.AD["KERNEL"]] = info["KERNEL"]      # TSD_AK_40_1 / _2 are the values that force them
    gout, ginfo = run(gpu_ctx, g, gops)             # the plain launch of the same instantiation on the gathered operands
    assert (ginfo["KERNEL"], ginfo["EXACT_WGS"]) == (info["KERNEL"], info["EXACT_WGS"])
    assert np.array_equal(out.view(np.uint16), A.pack_output(d, to_grid(A.unpack_output(g, gout), idx, B)).view(np.uint16))
    M, kw = (R, {}) if hd == 64 else (A, dict(kernel=info["KERNEL"]))
    pr, (fails, ratio) = M.predict_repeat(g, gops, **kw), M.check(g, gops, gout, **kw)
    must, may = int((pr == 1).sum()), int((pr == 0).sum())
    print(f"[attnwin] {IDS[i]}: worst error / bound {ratio:.3f}, exact repeats {info['EXACT_WGS']} (must {must}, may {may} more, of {pr.size})")
    assert not fails, "; ".join(fails)
    assert must <= info["EXACT_WGS"] <= must + may and (kind != "rising" or must >= 1), pr.tolist()


def test_keys_outside_the_window_do_not_matter(gpu_ctx):
    d, ops, _, _, idx = case(1)                      # d = 40, 16 x 16 windows of a 32 x 16 grid; everything outside window 1 at +-60000
    q, k, v, _ = (x.copy() for x in A.unpack_inputs(d, ops))
    outside = ~np.isin(np.arange(k.shape[2]), idx[1])
    sign = np.where(np.arange(k.shape[2]) % 2 == 0, 1.0, -1.0)[outside, None]
    k[:, :, outside], v[:, :, outside] = 60000.0 * sign, -60000.0 * sign
    a, b = (A.unpack_output(d, run(gpu_ctx, d, o)[0])[:, :, idx[1]] for o in (ops, A.pack(d, q, k, v)))
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


@pytest.fixture(scope="module")
def unet(gpu_ctx, tsd_mod):
    d = tsd_mod.Diffusion(params=draw_params(tsd_mod.param_specs(KIND), F.MODEL_SEED), variant=KIND)
    yield d
    d.model.close()


def model_inputs(LH, LW, B=2):
    """The shared draw at half weight on a +-1.5 checkerboard of 8 x 8 blocks: the NUMPY forward with windows is 0.25 (rel_l2) from the plain
    one at both shapes (0.07 - 0.09 on the bare draw, below the 10 TOL_MODEL asked of the device).  Odd samples are negated."""
    lat, ctx, temb = F.model_inputs(KIND, LH, LW)
    blocks = np.kron(np.where(np.add.outer(np.arange(-(-LH // 8)), np.arange(-(-LW // 8))) % 2 == 0, 1.5, -1.5), np.ones((8, 8)))[:LH, :LW]
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    return ((0.5 * lat + blocks) * sign[:, None, None, None]).astype(np.float32), np.repeat(ctx, B, 0), np.repeat(temb, B, 0)


@pytest.mark.parametrize("shape", F.MODEL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_with_a_window_table_matches_the_windowed_oracle(unet, tsd_mod, monkeypatch, shape):
    from oracle import ops
    E, idx, whole, own = tsd_mod._lib, win_index(WIN[0], *shape), ops.self_attention, (shape[0], shape[0] // 2, 0, 0)

    def windowed(x, *a, **kw):     # gather by window -> the oracle's self attention -> scatter, at the level-0 grid only
        if x.shape[0] != shape[0] * shape[1]:
            return whole(x, *a, **kw)
        y = np.empty_like(x)
        y[idx] = np.stack([whole(x[w], *a, **kw) for w in idx])
        return y

    lat, ctx, temb = model_inputs(*shape)
    plain = unet.forward(lat, ctx, temb)
    unet.set_attn_window(WIN[0])
    try:
        assert unet.attn_window == WIN
        out = unet.forward(lat, ctx, temb)
        three, alone = unet.forward(*model_inputs(*shape, B=3)), unet.forward(*model_inputs(*shape, B=1))
        unet.set_attn_window(own)                       # 16 x 16: every window is its grid - the bits of no table
        same = unet.forward(lat, ctx, temb)
        for bad in ((12, 0, 0, 0), (8, 0, 256, 0), (-8, 0, 0, 0)):      # a side outside the list: refused, the table stays
            with pytest.raises(tsd_mod.TsdError) as e:
                unet.set_attn_window(bad)
            assert e.value.code == E.TSD_E_ARG and unet.attn_window == own
        with pytest.raises(tsd_mod.TsdError) as e:      # 16 does not divide a 24-row grid: refused, never the whole grid silently
            unet.forward(*model_inputs(24, 16))
        assert e.value.code == E.TSD_E_SHAPE
    finally:
        unet.set_attn_window(None)
    monkeypatch.setattr(ops, "self_attention", windowed)
    P = draw_params(tsd_mod.param_specs(KIND), F.MODEL_SEED)
    ref = np.stack([F.diffusion_freeu(P, lat[b], ctx[b], temb[b], None, tn=True) for b in range(2)])
    assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, f"{KIND} {shape} window {WIN}")
    assert rel_l2(out, plain) > 10 * TOL_MODEL
    assert TC._same(three[2], alone[0]) and TC._same(out[0], alone[0])     # a sample alone and in position 2 of B = 3
    assert shape[0] != shape[1] or TC._same(same, plain)


def test_cfg_session_with_a_window_table_equals_the_host_loop_and_a_switch_acts_on_the_next_step(gpu_ctx, tsd_mod, unet):
    case, inputs = TC.S_CASES[0], TC._s_inputs(2300)          # seeded DDPM, CFG, 16 x 16 latents
    loop = lambda x0, first, n=1: TC.host_loop(tsd_mod, gpu_ctx, unet, None, case, True, inputs, lambda i: None, x0=x0, first=first, steps=first + n)
    s = TC._open(tsd_mod, unet, True, case[1], case[2], case[3])
    try:
        s.upload(inputs[0], inputs[1], inputs[2], None, cfg_scale=TC.S_CFG_SCALE)
        s.set_seeds(TC.S_SEEDS)
        s.step(0); g0 = s.latents()
        unet.set_attn_window(WIN)
        s.step(1); g1 = s.latents()
        s.close()
        w0, w1 = loop(None, 0, TC.S_STEPS), loop(g0, 1)[0]
        got = TC.session_run(tsd_mod, unet, None, case, True, inputs, None)
    finally:
        s.close()
        unet.set_attn_window(None)
    assert all(TC._same(a, b) for a, b in zip(got, w0)) and TC._same(g1, w1)
    assert TC._same(g0, loop(None, 0)[0]) and not TC._same(w1, loop(g0, 1)[0])


def test_generate_restores_the_table_and_other_kinds_are_refused(gpu_ctx, tsd_mod, unet):
    _, ctx, uctx, _, _ = TC._s_inputs(2310)
    kw = dict(uncond_context=uctx, cfg=True, cfg_scale=TC.S_CFG_SCALE, inference_steps=2, strength=1.0, L=TC.S_L, return_latents=True, seeds=TC.S_SEEDS)
    unet.set_attn_window((16, 8, 0, 0))              # what the model held before the calls (every window its grid)
    try:
        plain, out = tsd_mod.generate(unet, None, ctx, **kw), tsd_mod.generate(unet, None, ctx, attn_window=8, **kw)
        with pytest.raises(ValueError):              # a refused argument inside the call: the table is back as well
            tsd_mod.generate(unet, None, ctx, attn_window=8, controlnet=object(), **kw)
        stream = list(tsd_mod.generate_stream(unet, None, [tsd_mod.Request(0, ctx[0], uctx[0], seed=TC.S_SEEDS[0], cfg_scale=TC.S_CFG_SCALE)], 1, TC.S_L,
                                              inference_steps=2, attn_window=WIN))
        assert unet.attn_window == (16, 8, 0, 0) and not TC._same(out, plain) and TC._same(stream[0][1], out[0])
    finally:
        unet.set_attn_window(None)
    for other in (tsd_mod.Decoder(seed=1), tsd_mod.IPAdapter(seed=1)):      # neither a UNet nor a ControlNet
        assert tsd_mod._lib.lib().tsd_model_set_attn_window(other.model.h, None) == tsd_mod._lib.TSD_E_ARG
        other.model.close()
