"""LoRA merge on the device (csrc/kernels_lora.hip, tsd_model_lora_*), against the float64 reference `tsd.lora.merge_reference`.

(a) exact operands: bit-equal to the rounded float64 result, through every tiling edge, both layouts and the row interleave;
(b) general operands: inside [rn16(E - gamma), rn16(E + gamma)], gamma the any-order fp32 bound (lora_ref.gamma); the test prints
    the worst |d - E| / (ulp16/2 + gamma) of each shape - measured on an MI355X: 0.9497, 0.9974, 0.9923 (the rounding to fp16 is
    nearly all of it; gamma is 1e-4 to 1e-2 of the half ulp at these magnitudes);
(c) nothing but the addressed rows and real channels of the one parameter is written;
(d) lora_clear restores the bits, set_param makes a new base, a merge that leaves fp16 is refused and changes nothing;
(e) the forward reads the merged weights on every path the graph derives from them, and a session follows add / clear;
(f) load_lora end to end on the SD-1.x UNet, both key dialects."""
import numpy as np
import pytest

from lora_ref import (ATTN_SUFFIXES, as_state, attention_modules, check_interval, exact_operands, gamma, general_operands, merge_op,
                      unet_pairs)

pytestmark = pytest.mark.gpu

# (O, I, k, r, s, interleave, row0, rows)
EXACT_CASES = [
    (1, 1, 0, 1, 0.75, 0, 0, 1), (16, 16, 0, 4, -1.0, 0, 0, 16), (17, 65, 0, 5, 2.0, 0, 0, 17), (80, 96, 0, 33, 0.75, 0, 0, 80),
    (64, 320, 0, 64, -1.0, 0, 0, 64),
    (32, 70, 0, 5, 2.0, 1, 8, 16),        # GEGLU interleave: reference rows 8..23 hit both halves (16 is the first gate row)
    (4, 320, 3, 8, 0.75, 0, 0, 4), (320, 4, 3, 8, -1.0, 0, 0, 320), (3, 128, 3, 5, 2.0, 0, 0, 3),   # Opad > O, Ipad > I
    (40, 24, 1, 7, 0.75, 0, 0, 40),
    (50, 130, 0, 9, -1.0, 0, 7, 21),      # rows 7..27: starts and ends off any 16-row boundary
    (45, 20, 3, 6, 2.0, 0, 13, 19),       # the same for a convolution
]


def _shaped(W, I, k):
    return W.reshape(W.shape[0], I, k, k) if k else W


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "O%d_I%d_k%d_r%d_il%d_rows%d+%d" % (c[0], c[1], c[2], c[3], c[5], c[6], c[7]))
def test_merge_is_exact_on_exact_operands(tsd_mod, gpu_ctx, case):
    O, I, k, r, s, inter, row0, rows = case
    cols = I * (k * k if k else 1)
    W, up, down = exact_operands(O, cols, rows, r, seed=O * 131 + I)
    rc, out = merge_op(tsd_mod, gpu_ctx, _shaped(W, I, k), up, down, s, k=k, interleave=inter, row0=row0)
    assert rc == 0, tsd_mod._lib.last_error()
    out = out.reshape(O, cols)
    want = W.astype(np.float64)
    want[row0:row0 + rows] = tsd_mod.merge_reference(W[row0:row0 + rows], up, down, s)
    want16 = np.float16(want)
    assert np.array_equal(out.astype(np.float16).astype(np.float32), out)        # every value is an fp16
    bad = out.astype(np.float16).view(np.uint16) != want16.view(np.uint16)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} differ from rn16(float64), first at {np.argwhere(bad)[0]}"
    outside = np.ones(O, bool)
    outside[row0:row0 + rows] = False
    assert np.array_equal(out[outside], W[outside])                              # rows outside the range: the packed W, untouched


@pytest.mark.parametrize("O,I,r,s", [(64, 320, 128, 1.0), (40, 77, 5, -0.37), (16, 36, 1, 8.0)])
def test_merge_of_general_operands_stays_inside_the_fp32_interval(tsd_mod, gpu_ctx, O, I, r, s):
    W, up, down = general_operands(O, I, O, r, seed=O)
    rc, out = merge_op(tsd_mod, gpu_ctx, W, up, down, s)
    assert rc == 0, tsd_mod._lib.last_error()
    check_interval(out, tsd_mod.merge_reference(W, up, down, s), gamma(W, up, down, s), f"k_lora_merge {O}x{I} r={r} s={s}")


@pytest.fixture(scope="module")
def decoder(tsd_mod, gpu_ctx):
    m = tsd_mod.Model("decoder", ctx=gpu_ctx, seed=77)
    yield m
    m.close()


def _adapter(rows, r, cols, seed, amp=0.1):
    g = np.random.default_rng(seed)
    return (amp * g.standard_normal((rows, r))).astype(np.float32), (amp * g.standard_normal((r, cols))).astype(np.float32)


# decoder parameters: a 3x3 conv with Ipad > I (4 -> 512: Ipad 64), one with Opad > O (128 -> 3: Opad 4), a linear
DEC_CONV_IPAD, DEC_CONV_OPAD, DEC_LIN = "l2.kernel", "l26.kernel", "l4.attention.in_proj.weight"


@pytest.mark.parametrize("name,row0,rows", [(DEC_CONV_IPAD, 37, 100), (DEC_CONV_OPAD, 1, 2), (DEC_LIN, 513, 300)])
def test_lora_add_writes_only_the_addressed_rows_and_channels(tsd_mod, gpu_ctx, decoder, name, row0, rows):
    m = decoder
    m.lora_clear()
    i = m.param_index(name)
    shape = m.specs[i][1]
    O, I, kk = shape[0], shape[1], (shape[2] * shape[3] if len(shape) == 4 else 1)
    before = [m.packed_param(j) for j in (i - 1, i, i + 1)]
    w_before = m.get_param(i)
    up, down = _adapter(rows, 3, I * kk, seed=i)
    m.lora_add(name, up, down, 0.5, row0=row0)
    try:
        assert m.lora_count == 1
        after = [m.packed_param(j) for j in (i - 1, i, i + 1)]
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])   # the neighbours in the blob
        ld = 64 * ((I + 63) // 64)
        a16, b16 = (x.view(np.uint16).reshape(-1, kk, ld) for x in (after[1], before[1]))
        assert a16.shape[0] >= O and (kk == 1 or a16.shape[0] > O or ld > I)                  # the conv cases have pad rows or pad channels
        touched = np.zeros(a16.shape, bool)
        touched[row0:row0 + rows, :, :I] = True
        assert np.array_equal(a16[~touched], b16[~touched])
        assert (a16[touched] != b16[touched]).mean() > 0.5
        got = m.get_param(i).reshape(O, -1)
        wb = w_before.reshape(O, -1)
        assert np.array_equal(got[:row0], wb[:row0]) and np.array_equal(got[row0 + rows:], wb[row0 + rows:])
        check_interval(got[row0:row0 + rows], tsd_mod.merge_reference(wb[row0:row0 + rows], up, down, 0.5),
                       gamma(wb[row0:row0 + rows], up, down, 0.5), f"{name} rows {row0}+{rows}")
    finally:
        m.lora_clear()
    assert m.lora_count == 0 and np.array_equal(m.packed_param(i), before[1])


def test_lora_clear_restores_the_bits_and_refusals_change_nothing(tsd_mod, gpu_ctx, decoder):
    m = decoder
    m.lora_clear()
    names = (DEC_CONV_IPAD, DEC_CONV_OPAD, DEC_LIN)
    base = {n: m.packed_param(n) for n in names}
    orig_lin = m.get_param(DEC_LIN)
    for n in names:
        shape = m.specs[m.param_index(n)][1]
        for rep in range(2):                              # two stacked adds on each of three parameters
            up, down = _adapter(shape[0], 2 + rep, int(np.prod(shape[1:])), seed=rep)
            m.lora_add(n, up, down, 1.0 - 1.5 * rep)
    assert m.lora_count == 3 and all(not np.array_equal(m.packed_param(n), base[n]) for n in names)
    m.lora_clear()
    assert m.lora_count == 0
    for n in names:
        assert np.array_equal(m.packed_param(n), base[n]), n
    # set_param on a touched parameter: the new value is the new base, lora_clear keeps it
    shape = m.specs[m.param_index(DEC_LIN)][1]
    up, down = _adapter(shape[0], 2, shape[1], seed=9)
    m.lora_add(DEC_LIN, up, down, 1.0)
    m.lora_add(DEC_CONV_OPAD, *_adapter(3, 2, 128 * 9, seed=10), 1.0)
    new = (0.01 * np.random.default_rng(3).standard_normal(shape)).astype(np.float16).astype(np.float32)
    m.set_param(m.param_index(DEC_LIN), new)
    assert m.lora_count == 1
    m.lora_clear()
    assert m.lora_count == 0 and np.array_equal(m.get_param(DEC_LIN), new) and np.array_equal(m.packed_param(DEC_CONV_OPAD), base[DEC_CONV_OPAD])
    m.set_param(m.param_index(DEC_LIN), orig_lin)         # (every weight read back is an fp16: setting it again reproduces the bits)
    assert np.array_equal(m.packed_param(DEC_LIN), base[DEC_LIN])
    # a merge that leaves fp16 is refused: bytes, snapshots and count as before, and the next call is not poisoned
    m.lora_add(DEC_CONV_IPAD, *_adapter(512, 2, 36, seed=12), 1.0)
    held = {n: m.packed_param(n) for n in names}
    ones = np.ones((3, 4), np.float32), np.ones((4, 128 * 9), np.float32)
    for n, (up, down), s in ((DEC_CONV_OPAD, ones, 1e6), (DEC_CONV_IPAD, (np.ones((512, 4), np.float32), np.ones((4, 36), np.float32)), 1e6),
                             (DEC_CONV_OPAD, (ones[0], np.full((4, 128 * 9), np.inf, np.float32)), 1.0)):
        with pytest.raises(tsd_mod.TsdError) as e:
            m.lora_add(n, up, down, s)
        assert e.value.code == tsd_mod._lib.TSD_E_NONFINITE
        assert m.lora_count == 1 and all(np.array_equal(m.packed_param(k), held[k]) for k in names)
    gpu_ctx.synchronize()                                 # the count was reported once and cleared
    m.lora_add(DEC_CONV_OPAD, ones[0], ones[1], 1e-3)
    assert m.lora_count == 2
    m.lora_clear()
    assert all(np.array_equal(m.packed_param(n), base[n]) for n in names)
    # refusals of the arguments
    E = tsd_mod._lib
    for args, code in (((DEC_CONV_OPAD, ones[0], ones[1], np.inf), E.TSD_E_ARG), (("l26.bias", ones[0], ones[1], 1.0), E.TSD_E_ARG),
                       ((DEC_CONV_OPAD, ones[0], ones[1], 1.0, 1), E.TSD_E_SHAPE), ((DEC_CONV_OPAD, ones[0], ones[1], 1.0, -1), E.TSD_E_SHAPE),
                       (("l3.res_conv_layer.kernel", np.ones((512, 1), np.float32), np.ones((1, 512), np.float32), 1.0), E.TSD_E_ARG)):  # never read: 512 -> 512
        with pytest.raises(tsd_mod.TsdError) as e:
            m.lora_add(*args)
        assert e.value.code == code, args[0]
    fresh = tsd_mod.Model("decoder", ctx=gpu_ctx)
    with pytest.raises(tsd_mod.TsdError) as e:
        fresh.lora_add(DEC_CONV_OPAD, ones[0], ones[1], 1.0)
    assert e.value.code == E.TSD_E_STATE and m.lora_count == 0
    fresh.close()


def test_forward_and_session_read_the_merged_weights(tsd_mod, gpu_ctx):
    from oracle import ops, rng
    seed, B, L, T = 4321, 1, 8, 77
    lat = rng.normal(seed, 1, B * 4 * L * L).reshape(B, 4, L, L)
    ctx = rng.normal(seed, 2, B * T * 768).reshape(B, T, 768)
    noise = rng.normal(seed, 3, 2 * B * 4 * L * L).reshape(2, B, 4, L, L)
    temb = ops.time_embedding(500.0)
    A = tsd_mod.Diffusion(seed=seed, ctx=gpu_ctx)
    base_out = A.forward(lat, ctx, temb)
    # one parameter of each kind the graph treats specially: (name, row0, rows or None = all)
    C6 = 640
    touched = [("unet.layer2.layer3.weight", 0, None),           # region 1: row block of the concatenated time projection
               ("unet.layer6.layer6.k_proj.weight", 0, None),    # region 3: row block of the concatenated context k_proj
               ("unet.layer3.layer8.weight", 100, 2400),         # GEGLU row interleave, both halves; the fused tail kernel's stream
               ("unet.layer6.layer4.in_proj.weight", C6, C6),    # the k rows of a stacked in_proj
               ("unet.layer10.layer2.kernel", 0, None),          # duplicate-concat fold
               ("unet.layer15.layer2.kernel", 0, None),          # upsample fold
               ("unet.layer9.layer9.weight", 0, None), ("unet.layer9.layer10.kernel", 0, None)]   # GEGLU-2 / conv_out fold
    m = A.model
    base_bytes = {name: m.packed_param(name) for name, _, _ in touched}
    for j, (name, row0, rows) in enumerate(touched):
        shape = m.specs[m.param_index(name)][1]
        up, down = _adapter(rows or shape[0], 4, int(np.prod(shape[1:])), seed=j, amp=0.05)
        m.lora_add(name, up, down, 1.0, row0=row0)
    assert m.lora_count == len(touched)
    out_a = A.forward(lat, ctx, temb)
    assert np.isfinite(out_a).all() and not np.array_equal(out_a, base_out)
    Bm = tsd_mod.Model("diffusion", ctx=gpu_ctx)
    for i in range(len(m.specs)):
        Bm.set_param(i, m.get_param(i))
    Bd = tsd_mod.Diffusion.__new__(tsd_mod.Diffusion)
    Bd.model = Bm
    assert np.array_equal(Bd.forward(lat, ctx, temb), out_a)     # the derived buffers were rebuilt from the merged weights
    Bm.close()
    # a session follows: step(0) on the merged weights, lora_clear, step(1) on the base through the existing generation check
    sess = tsd_mod.Session(m, None, B, L, T)
    sess.set_schedule(1000, 2, 0)
    sess.upload(lat, ctx, None, noise)
    sess.step(0)
    lat0 = sess.latents()
    m.lora_clear()
    assert m.lora_count == 0
    for name, _, _ in touched:                                   # (up to 59 MB each: the snapshot copy is ordered with the merge's copy)
        assert np.array_equal(m.packed_param(name), base_bytes[name]), name
    sess.step(1)
    lat1 = sess.latents()
    sess.close()
    assert np.array_equal(A.forward(lat, ctx, temb), base_out)   # cleared: the base model's bits again
    F = tsd_mod.Diffusion(seed=seed, ctx=gpu_ctx)
    fs = tsd_mod.Session(F.model, None, B, L, T)
    fs.set_schedule(1000, 2, 0)
    fs.upload(lat, ctx, None, noise)
    fs.step(0)
    assert not np.array_equal(fs.latents(), lat0)                # step(0) of the session above ran the adapter
    fs.upload(lat0, ctx, None, noise)
    fs.step(1)
    assert np.array_equal(fs.latents(), lat1)
    fs.close()
    F.model.close()
    m.close()


def test_load_lora_end_to_end_on_the_sd15_unet(tsd_mod, gpu_ctx):
    unet = tsd_mod.Diffusion(seed=5, ctx=gpu_ctx, variant="diffusion_sd15_torch")
    m = unet.model
    mods = [f"{a}.{s}" for a in attention_modules(tsd_mod) for s in ATTN_SUFFIXES] + ["down_blocks.2.resnets.0.conv1"]
    assert len(mods) == 16 * 12 + 1
    rank, alpha = 4, 2.0
    pairs = unet_pairs(tsd_mod, mods, rank, seed=21)
    te = as_state({"text_model.encoder.layers.0.mlp.fc1": (np.zeros((rank, 768), np.float32), np.zeros((3072, rank), np.float32))}, "kohya", alpha, "text_encoder")
    targets = tsd_mod.lora_targets("diffusion_sd15_torch")
    by_param = {}
    for mod in mods:
        by_param.setdefault(targets[mod][0], []).append(mod)
    before = {p: m.get_param(p) for p in by_param}
    res = tsd_mod.load_lora(dict(as_state(pairs, "kohya", alpha), **te), unet=unet)
    assert res == {"applied": len(pairs), "skipped": ["text_encoder.text_model.encoder.layers.0.mlp.fc1"]} and m.lora_count == len(by_param)
    s = alpha / rank
    packed = {}
    for p, ms in by_param.items():
        W = before[p].reshape(before[p].shape[0], -1)
        got = m.get_param(p).reshape(W.shape)
        E, g = W.astype(np.float64), np.zeros(W.shape)
        for mod in ms:                                     # q / k / v land in disjoint row blocks of one in_proj: one rounding per row
            _, row0, rows = targets[mod]
            down, up = pairs[mod]
            E[row0:row0 + rows] = tsd_mod.merge_reference(W[row0:row0 + rows], up, down, s)
            g[row0:row0 + rows] = gamma(W[row0:row0 + rows], up.reshape(rows, -1), down, s)
        assert sum(targets[mod][2] for mod in ms) == W.shape[0]
        d = got.astype(np.float64)
        out = int(((d < np.float16(E - g)) | (d > np.float16(E + g))).sum())
        assert out == 0, f"{p}: {out} of {d.size} merged weights leave the interval"
        assert not np.array_equal(got, W)
        packed[p] = m.packed_param(p)
    # the PEFT spelling of the same adapter gives the same bytes
    m.lora_clear()
    assert m.lora_count == 0 and all(np.array_equal(m.get_param(p), before[p]) for p in list(by_param)[:3])
    res = tsd_mod.load_lora(as_state(pairs, "peft", alpha), unet=m)
    assert res == {"applied": len(pairs), "skipped": []}
    for p in by_param:
        assert np.array_equal(m.packed_param(p), packed[p]), p
    m.close()
