"""Shared self attention (flash_attn_share_kernel) through version-4 descriptors of tsd_debug_attn_run, held to fp64 and to the plain
launches' bits, run to run and under the jitter build; and the table of a kind-6 model, its sessions and generate(reference_image=)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attn64_ref as R
import attn_ref as A
import attnshare_ref as S
import replay
import test_gpu_controlnet as TC      # the host loop and the session driver; its bitwise comparison
from test_gpu_attnwin import model_inputs, unet  # noqa: F401  (the kind-6 model on the shared draw, and its checkerboard inputs)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITTER_LIB = os.path.join(ROOT, "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
CHILD = "import json, sys; sys.path[:0] = %r; import tsd, test_gpu_attnshare as T; tsd.set_strict(True); print(json.dumps(T.bitwise_cases(tsd, %d)))"
JITTER_REPEATS, JITTER_CASES = 3, (3, 4)      # d = 40 QB = 2 at nine tiles a segment; d = 64 with a masked tail in the middle
KIND, TABLE, same = "diffusion_sd15_torch", (-1, 0, 0), TC._same
RUNS = [(i, "flat") for i in range(len(S.CASES))] + [(i, "spike") for i, c in enumerate(S.CASES) if c[4] % 64 == 0]


def run(ctx, d, ops):
    rc, outs, info = replay.run("tsd_debug_attn_run", ctx, d, ops, A.AO, A.INPUTS, ("O",), A.dtype_of, A.extents)
    assert rc == 0, replay.lib().tsd_last_error().decode()
    return outs["O"], {k: int(info[v]) for k, v in A.AI.items() if k != "COUNT"}


@pytest.mark.parametrize("i, kind", RUNS, ids=[f"{S.IDS[i]}-{k}" for i, k in RUNS])
def test_every_sample_is_inside_the_fp64_bound_and_has_the_plain_launch_bits(gpu_ctx, i, kind):
    (hd, kern, H, table, s), (base, d, ops) = S.CASES[i], S.case(i, kind)
    out, info = run(gpu_ctx, d, ops)
    o = A.unpack_output(d, out)
    plain, pinfo = run(gpu_ctx, base, ops)                # nobody shares: the version-2 launch of the same instantiation
    assert info["CHANGED"] == 0 and info["KERNEL"] == pinfo["KERNEL"] and info["DIAG"] == A.F(base, "DIAG")
    replay.assert_gaps_hold_fill(out, A.o_index(d), "O")
    M, exact, worst = (R if hd == 64 else A), 0, 0.0
    for b, t in enumerate(table):
        g, gops = S.gathered(base, ops, b, t)
        kw = {} if hd == 64 else dict(kernel=info["KERNEL"])
        fails, ratio = M.check(g, gops, A.pack_output(g, o[b:b + 1]), **kw)
        assert not fails, f"sample {b}: " + "; ".join(fails)
        worst = max(worst, ratio)
        if t < 0:                                         # bit for bit the plain run, at every S, whoever reads this sample's keys
            assert same(o[b], A.unpack_output(base, plain)[b]), b
        elif s % 64 == 0:                                 # whole tiles: the plain launch over the gathered 2 S keys, bits and repeats
            gout, ginfo = run(gpu_ctx, g, gops)
            assert ginfo["KERNEL"] == info["KERNEL"] and same(o[b], A.unpack_output(g, gout)[0]), b
            pr = M.predict_repeat(g, gops, **kw)
            assert kind != "spike" or ((pr == 1).all() and ginfo["EXACT_WGS"] == pr.size), (b, pr.tolist())      # 30 log2 units up in segment 1
            exact += ginfo["EXACT_WGS"]
    print(f"[attnshare] {S.IDS[i]} {kind}: worst error / bound {worst:.3f}, exact repeats {info['EXACT_WGS']}")
    # without sharing nobody repeats (a spike sits in segment 1 only), so the samples without an entry, bitwise their plain run, add none
    assert pinfo["EXACT_WGS"] == 0 and (s % 64 or info["EXACT_WGS"] == exact)
    if s == 4:                                            # V^T pad columns 4 .. 7 of either segment at +-60000 change no bit
        q, k, v, _ = A.unpack_inputs(base, ops)
        padded = run(gpu_ctx, d, A.pack(base, q, k, v, A.pad_fill(base)))[0]
        assert np.array_equal(padded[A.o_index(d)].view(np.uint16), out[A.o_index(d)].view(np.uint16))


def bitwise_cases(tsd, repeats):
    c = tsd.default_context()
    return [[hashlib.sha256(run(c, *S.case(i)[1:])[0].tobytes()).hexdigest() for _ in range(repeats)] for i in JITTER_CASES]


def test_same_bits_run_to_run_and_under_the_jitter_build(tsd_mod, gpu_ctx):
    here = bitwise_cases(tsd_mod, 3)
    assert all(len(set(d)) == 1 for d in here), here
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    paths = [os.path.join(ROOT, "tests"), ROOT, os.path.dirname(os.path.dirname(JITTER_LIB))]      # a fresh process on the jitter library
    out = subprocess.run([sys.executable, "-c", CHILD % (paths, JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = json.loads(out.stdout.strip().splitlines()[-1])
    assert [len(d) for d in there] == [JITTER_REPEATS] * len(here) and all(set(t) == set(h) for t, h in zip(there, here)), (there, here)


@pytest.mark.parametrize("shape", [(16, 16), (16, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_with_a_share_table_matches_the_numpy_forward_over_concatenated_keys(unet, tsd_mod, monkeypatch, shape):
    import freeu_ref as F
    from controlnet_ref import draw_params
    from oracle import ops
    from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, rel_l2
    lat, ctx, temb = model_inputs(*shape, B=3)        # the shared draw on a checkerboard, odd samples negated
    lat[1:] *= 0.3                                    # the sharers at 0.3 of the reference's amplitude, so that its keys weigh
    plain = unet.forward(lat, ctx, temb)
    unet.set_attn_share(TABLE)
    try:
        out = unet.forward(lat, ctx, temb)
    finally:
        unet.clear_attn_share()
    assert unet.attn_share is None and same(unet.forward(lat, ctx, temb), plain)      # off after on: the never-set bits
    whole, seen = ops.self_attention, []

    def recording(x, *a, **kw):            # sample 0 runs first and leaves the input of every self attention behind
        seen.append(x)
        return whole(x, *a, **kw)

    def shared(x, H, w_in, b_in, w_out, b_out, causal=False, sem=ops.DEFAULT):      # q from x, keys and values from [x ; the reference's x]
        q = np.split(ops.linear(x, w_in, b_in), 3, axis=-1)[0]
        _, k, v = np.split(ops.linear(np.concatenate([x, todo.pop(0)]), w_in, b_in), 3, axis=-1)
        return ops.linear(ops.attention_core(q, k, v, H, causal, sem), w_out, b_out)

    P, ref = draw_params(tsd_mod.param_specs(KIND), F.MODEL_SEED), []
    for b in range(3):
        todo = list(seen)
        monkeypatch.setattr(ops, "self_attention", shared if b else recording)
        ref.append(F.diffusion_freeu(P, lat[b], ctx[b], temb[b], None, tn=True))
    print(f"[attnshare] {KIND} {shape}: {rel_l2(out, np.stack(ref)):.2e} from the numpy forward, {rel_l2(out, plain):.2e} from the plain forward")
    assert_close(out, np.stack(ref), TOL_MODEL, TOL_MODEL_MAX, f"{KIND} {shape} share {TABLE}")
    assert rel_l2(out, plain) >= 3 * TOL_MODEL and same(out[0], plain[0])      # over the WHOLE output, sample 0's exact zero included


def test_refusals_leave_the_table_as_it_was(unet, tsd_mod):
    E, held = tsd_mod._lib, dict(share=TABLE, levels=(0, 1, 1, 1), cond_only=False)
    unet.set_attn_share(**held)
    unet.set_attn_window(8)
    try:
        for call in ([unet.set_attn_share, (0, -1)], [unet.set_attn_share, (-1, 2)], [unet.set_attn_share, (-1,) + (0,) * 32],
                     [unet.set_attn_share, TABLE], [unet.set_attn_window, (0, 8, 0, 0)], [unet.set_token_merge, (0, 0.5, 0, 0)]):
            with pytest.raises(tsd_mod.TsdError) as e:      # own index, >= n, n > 32; a level has a window, a ratio or sharing, never two
                call[0](call[1])
            assert e.value.code == E.TSD_E_ARG and unet.attn_share == held
        dec = tsd_mod.Decoder(seed=1)
        assert E.lib().tsd_model_set_attn_share(dec.model.h, None, 0, None, 0) == E.TSD_E_ARG      # no UNet
        dec.model.close()
    finally:
        unet.clear_attn_share()
        unet.set_attn_window(None)


def test_cond_only_cfg_session_equals_the_host_loop_and_a_switch_acts_on_the_next_step(gpu_ctx, tsd_mod, unet, monkeypatch):
    monkeypatch.setattr(TC, "S_B", 2)       # test_gpu_controlnet's drivers at B = 2: the UNet runs [cond 0, cond 1 ; uncond 0, uncond 1]
    monkeypatch.setattr(TC, "S_SEEDS", [777, 778])
    case, inputs = TC.S_CASES[0], TC._s_inputs(2400)          # seeded DDPM, CFG, 16 x 16 latents; sample 1 reads sample 0, conditional half only
    loop = lambda x0, first, n=1: TC.host_loop(tsd_mod, gpu_ctx, unet, None, case, True, inputs, lambda i: None, x0=x0, first=first, steps=first + n)
    s = TC._open(tsd_mod, unet, True, case[1], case[2], case[3])
    try:
        s.upload(inputs[0], inputs[1], inputs[2], None, cfg_scale=TC.S_CFG_SCALE)
        s.set_seeds(TC.S_SEEDS)
        s.step(0); g0 = s.latents()
        unet.set_attn_share((-1, 0), cond_only=True)
        s.step(1); g1 = s.latents()
        s.close()
        w0, w1 = loop(None, 0, TC.S_STEPS), loop(g0, 1)[0]
        got = TC.session_run(tsd_mod, unet, None, case, True, inputs, None)
    finally:
        s.close()
        unet.clear_attn_share()
    assert len(got) == TC.S_STEPS and all(same(a, b) for a, b in zip(got, w0)) and same(g1, w1)
    assert same(g0, loop(None, 0)[0]) and not same(w1, loop(g0, 1)[0])


def test_generate_with_a_reference_image_is_the_explicit_session_and_restores_the_table(gpu_ctx, tsd_mod, unet, monkeypatch):
    monkeypatch.setattr(TC, "S_B", 2)
    monkeypatch.setattr(TC, "S_SEEDS", [777, 778])
    from oracle import rng
    from tsd.utils import latent_mask, rescale
    (_, ctx, uctx, _, _), L, enc, seeds = TC._s_inputs(2410), TC.S_L, tsd_mod.Encoder(seed=3), TC.S_SEEDS
    img = 255 * rng.uniform(7, 2420, 3 * 3 * 64 * L * L, 0.5).reshape(3, 3, 8 * L, 8 * L) + 127.5
    mask = np.zeros((2, 8 * L, 8 * L), np.float32)
    mask[:, :, :4 * L] = 1.0                # the caller's own inpainting mask on the two samples: the left half is regenerated
    kw = dict(uncond_context=uctx, cfg=True, cfg_scale=7.5, inference_steps=3, L=L, return_latents=True, seeds=seeds)
    unet.set_attn_share((-1, 0), levels=(0, 1, 0, 0))                # what the model holds before the call, and again after it
    s = tsd_mod.Session(unet.model, None, 3, L, TC.T, cfg=True)      # the explicit session at B + 1: the reference last
    try:
        got = tsd_mod.generate(unet, None, ctx, input_image=img[:2], mask=mask, encoder=enc, strength=0.7, reference_image=img[2], **kw)
        assert unet.attn_share == dict(share=(-1, 0), levels=(0, 1, 0, 0), cond_only=False)
        known = np.concatenate([enc.forward(rescale(img[:2], (0, 255), (-1, 1)), rng.normal(0, 1, 8 * L * L).reshape(2, 4, L, L)),
                                enc.forward(rescale(img[2:], (0, 255), (-1, 1)), rng.normal(0, 5, 4 * L * L).reshape(1, 4, L, L))])
        s.set_schedule(1000, 3, 3 - int(3 * 0.7))
        s.upload(known, np.concatenate([ctx, ctx[:1]]), np.concatenate([uctx, uctx[:1]]), None, 7.5)
        s.set_seeds(seeds + [seeds[-1] + 1])
        s.add_noise_seeded(0)               # the reference under an all-zero mask, seeded, sharing (2, 2, -1) in the conditional half
        s.set_inpaint(np.concatenate([latent_mask(mask, "any", gpu_ctx), np.zeros((1, L, L), np.float32)]), known, seeded=True)
        unet.set_attn_share((2, 2, -1), cond_only=True)
        for i in range(s.num_steps):
            s.step(i)
        assert same(got, s.latents()[:2])
    finally:
        s.close()
        enc.model.close()
        unet.clear_attn_share()
