"""GPU: IP-Adapter Plus (model kind 24).  (1) `resample` - the Perceiver resampler, existing kernels only (csrc/graph.cpp g_ip_resample) -
against the fp64 restatement of tests/ipplus_ref.py at (B, S) = (1, 1), (2, 5), (2, 48), (3, 49), (2, 257): S + 16 = 64 / 65 sit at the
flash kernel's 64-key tile edge, 17 / 21 / 273 are no multiples of 8.  (2) finite garbage in the workspace (two contexts whose arena is
poisoned with different bytes, and whatever an earlier call of another shape left behind) changes no bit.  (3) run to run, batch
position and the jitter build are bitwise.  (4) the refusals leave tokens_out untouched.  (5) the adapted forward of the full-size UNet
on the 16 resampled tokens against the numpy restatement.  (6) a session equals the host-driven loop bitwise.  (7) `generate` from
pixels equals `generate` from hidden states and the explicit session loop.

Measured against the fp64 reference on an MI355X (tolerance 1e-2 relative L2 / 1.2e-2 of the largest value): resample 8.0e-4 / 9.1e-4 at
(1, 1), 9.2e-4 / 9.1e-4 at (2, 5), 1.10e-3 / 1.26e-3 at (2, 48), 1.11e-3 / 1.09e-3 at (3, 49), 1.01e-3 / 1.04e-3 at (2, 257); the adapted
forward 1.4e-3 / 1.2e-3, and 0.37 from the plain forward; the jitter build gave the shipped digest in 8 of 8 repeats."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # the jitter child: the repository root (oracle) and the package before the reference modules load
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "stable-diffusion.mojo_amd")]

import ipplus_ref as R
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, max_rel, rel_l2

pytestmark = pytest.mark.gpu
KIND = "ip_adapter_plus_sd15"
DRAW_SEED = 3
SHAPES = ((1, 1), (2, 5), (2, 48), (3, 49), (2, 257))
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
JITTER_REPEATS, JITTER_SHAPE = 8, (2, 49)


def hidden_of(B, S):
    return R.hidden_states(B, S, 4200 + 17 * S + B)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class Plus:
    """One adapter from the test draw, its parameters as the engine holds them, and the fp64 reference of every shape, computed once."""

    def __init__(self, tsd_mod):
        self.draw = R.draw_params(DRAW_SEED)
        self.ip = tsd_mod.IPAdapter(variant=KIND, params=self.draw)
        self.P = {n: self.ip.model.get_param(n) for n, *_ in tsd_mod.param_specs(KIND)}
        self._ref = {}

    def ref(self, B, S):
        if (B, S) not in self._ref:
            r = R.resample_batch(self.P, hidden_of(B, S))
            r.setflags(write=False)
            self._ref[(B, S)] = r
        return self._ref[(B, S)]


@pytest.fixture(scope="module")
def plus(gpu_ctx, tsd_mod):
    p = Plus(tsd_mod)
    yield p
    p.ip.model.close()


# ---- 1. the resampler against the fp64 reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", SHAPES, ids=[f"B{b}_S{s}" for b, s in SHAPES])
def test_resample_matches_the_fp64_reference(plus, B, S):
    assert plus.ip.n_tokens == 16 and plus.ip.is_plus
    # the engine holds the draw rounded to fp16 (matrices, latents) and unchanged (vectors)
    assert np.array_equal(plus.P["image_proj.latents"], plus.draw["image_proj.latents"].astype(np.float16).astype(np.float32))
    assert np.array_equal(plus.P["image_proj.layers.1.1.0.bias"], plus.draw["image_proj.layers.1.1.0.bias"])
    h = hidden_of(B, S)
    tok = plus.ip.resample(h)
    ref = plus.ref(B, S)
    print(f"[ipplus] resample B = {B} S = {S}: rel_l2 {rel_l2(tok, ref):.3e}, max error / max |ref| {max_rel(tok, ref):.3e}")
    assert tok.shape == (B, 16, 768) and tok.dtype == np.float32
    assert_close(tok, ref, TOL_MODEL, TOL_MODEL_MAX, f"resample B={B} S={S}")
    assert np.array_equal(tok.astype(np.float16).astype(np.float32), tok), "a token value is not an fp16"
    np.testing.assert_array_equal(plus.ip.resample(h[0]), tok[0])      # the (S, 1280) form


# ---- 2. finite garbage in the pad ---------------------------------------------------------------------------------------------------------
# The graph reads exactly B * S rows of `hidden`, so nothing of a larger host buffer reaches it; what it leaves unwritten by a kernel are
# the rows S + 16 .. Sp - 1 of every sample's key block (zeroed by a memset each call) and, derived from them, the K rows and V^T columns
# past S + 16.  The workspace they live in is the context's arena: TSD_DEBUG_POISON fills a fresh arena with a byte (0x3c3c = 1.06,
# 0x5a5a = 203 as fp16, both finite), and an earlier call of another shape leaves its own finite data there.
@pytest.mark.parametrize("B,S", ((2, 5), (3, 49)), ids=["B2_S5", "B3_S49"])
def test_finite_garbage_in_the_workspace_changes_no_bit(plus, tsd_mod, gpu_ctx, B, S):
    h = hidden_of(B, S)
    want = plus.ip.resample(h)
    plus.ip.resample(hidden_of(2, 257))                       # a larger call writes all over the arena ...
    assert _same(plus.ip.resample(h), want)                   # ... and the smaller one after it gives the same bits
    prev = os.environ.get("TSD_DEBUG_POISON")
    try:
        for byte in (0x3C, 0x5A):
            os.environ["TSD_DEBUG_POISON"] = str(byte)
            c = tsd_mod.Context(gpu_ctx.device)
            ip = tsd_mod.IPAdapter(variant=KIND, params=plus.draw, ctx=c)
            try:
                assert _same(ip.resample(h), want), f"arena poison 0x{byte:02x} reached the result"
            finally:
                ip.model.close()
                c.close()
    finally:
        if prev is None:
            os.environ.pop("TSD_DEBUG_POISON", None)
        else:
            os.environ["TSD_DEBUG_POISON"] = prev


# ---- 3. bitwise ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (49, 257))
def test_run_to_run_and_batch_position_are_bitwise(plus, S):
    h3 = hidden_of(3, S)
    y3 = plus.ip.resample(h3)
    assert _same(plus.ip.resample(h3), y3)
    for src in range(3):
        alone = plus.ip.resample(h3[src:src + 1])[0]
        assert _same(alone, y3[src]), (S, src)
        for pos in range(3):
            order = [(src + j - pos) % 3 for j in range(3)]
            assert _same(plus.ip.resample(h3[order])[pos], alone), (S, src, pos)


def jitter_digests(ip, repeats):
    h = hidden_of(*JITTER_SHAPE)
    return [hashlib.sha256(np.ascontiguousarray(ip.resample(h)).view(np.uint32).tobytes()).hexdigest()[:16] for _ in range(repeats)]


def test_jitter_build_reproduces_the_shipped_bits(plus):
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    here = jitter_digests(plus.ip, 1)[0]
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(there) == 1 and len(there[0]["digests"]) == JITTER_REPEATS
    assert all(dg == here for dg in there[0]["digests"]), f"the jitter build gave {len(set(there[0]['digests']))} result(s), not the shipped bits"


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_tokens_out_untouched(plus, unet, tsd_mod, gpu_ctx):
    from tsd._lib import f32, lib, ptr
    E = tsd_mod._lib
    h = f32(hidden_of(1, 5))
    big = f32(np.zeros((17, 1, 1280), np.float32))
    sentinel = np.float32(-12345.5)

    def call(model, hidden, B, S, fn="tsd_ip_adapter_resample"):
        out = np.full((max(B, 1), 16, 768), sentinel, np.float32)
        rc = getattr(lib(), fn)(model.h, ptr(hidden), B, S, ptr(out)) if fn == "tsd_ip_adapter_resample" else getattr(lib(), fn)(model.h, ptr(hidden), B, ptr(out))
        assert (out == sentinel).all(), f"{fn} B={B} S={S}: tokens_out was written"
        return rc
    assert call(plus.ip.model, h, 0, 5) == E.TSD_E_SHAPE
    assert call(plus.ip.model, big, 17, 1) == E.TSD_E_SHAPE
    assert call(plus.ip.model, h, 1, 0) == E.TSD_E_SHAPE
    assert call(plus.ip.model, h, 1, 1025) == E.TSD_E_SHAPE
    plain = tsd_mod.IPAdapter(seed=9)
    assert call(plain.model, h, 1, 5) == E.TSD_E_ARG                                   # a kind-20 model has no resampler
    assert "tsd_ip_adapter_project" in E.last_error()
    emb = f32(np.zeros((1, 1024), np.float32))
    assert call(plus.ip.model, emb, 1, 0, fn="tsd_ip_adapter_project") == E.TSD_E_ARG  # ... and a kind-24 model no linear projection
    assert "tsd_ip_adapter_resample" in E.last_error()
    with pytest.raises(tsd_mod.TsdError, match="tsd_ip_adapter_resample"):
        plus.ip.project(emb)
    with pytest.raises(tsd_mod.TsdError, match="tsd_ip_adapter_project"):
        plain.resample(h)
    with pytest.raises(ValueError):
        plus.ip.resample(np.zeros((5, 1024), np.float32))
    d = unet
    with pytest.raises(tsd_mod.TsdError) as e:                                         # lora_add answers as for kind 20
        plus.ip.model.lora_add("ip_adapter.1.to_k_ip.weight", np.zeros((320, 2), np.float32), np.zeros((2, 768), np.float32), 1.0)
    assert e.value.code == E.TSD_E_ARG
    assert lib().tsd_model_context_width(plus.ip.model.h) == lib().tsd_model_context_width(plain.model.h)
    # a plus adapter on another context: refused by the forward and by the session
    c2 = tsd_mod.Context(gpu_ctx.device)
    far = tsd_mod.IPAdapter(variant=KIND, seed=1, ctx=c2)
    tok = plus.ip.resample(hidden_of(2, 5))
    lat = np.zeros((2, 4, 16, 16), np.float32)
    cx = np.zeros((2, 77, 768), np.float32)
    temb = np.zeros((2, 320), np.float32)
    with pytest.raises(tsd_mod.TsdError) as e:
        d.forward(lat, cx, temb, ip_adapter=far, ip_tokens=tok)
    assert e.value.code == E.TSD_E_ARG
    s = tsd_mod.Session(d.model, None, 2, 16, 77, cfg=False)
    s.set_schedule(1000, 3, 0)
    s.upload(lat, cx, None, None)
    with pytest.raises(tsd_mod.TsdError) as e:
        s.set_ip_adapter(far, tok)
    assert e.value.code == E.TSD_E_ARG and not s.ip_adapter_active
    s.close()
    far.model.close(); c2.close(); plain.model.close()


# ---- 5. the adapted forward on 16 tokens -----------------------------------------------------------------------------------------------------
SEED, T, IP_SCALES = 1234, 77, (1.0, 0.6)


@pytest.fixture(scope="module")
def unet(gpu_ctx, tsd_mod):
    d = tsd_mod.Diffusion(seed=SEED, variant="diffusion_sd15")
    yield d
    d.model.close()


def test_adapted_forward_on_the_resampled_tokens(plus, unet, tsd_mod):
    import controlnet_ref as CR
    import ipadapter_ref as IR
    from oracle import ops, rng, spec
    B, LH, LW, S = 2, 16, 16, 49
    lat = rng.normal(7, 2100, B * 4 * LH * LW).reshape(B, 4, LH, LW)
    cx = rng.normal(7, 2101, B * T * 768).reshape(B, T, 768)
    temb = np.stack([ops.time_embedding(t) for t in (980.0, 20.0)])
    h = hidden_of(B, S)
    tok = plus.ip.resample(h)
    assert tok.shape == (B, 16, 768)
    tok_ref = R.resample_batch(plus.P, h).astype(np.float32)
    PU = spec.init_params("diffusion_sd15", SEED, only_used=True)
    ref = []
    for b in range(B):
        with IR.adapted(PU, plus.P, tok_ref[b], IP_SCALES[b]):
            ref.append(CR.diffusion_sd15_controlled(PU, lat[b], cx[b], temb[b], None, 0.0, tn=False))
    del PU
    ref = np.stack(ref)
    out = unet.forward(lat, cx, temb, ip_adapter=plus.ip, ip_tokens=tok, ip_scale=IP_SCALES)
    plain = unet.forward(lat, cx, temb)
    print(f"[ipplus] adapted forward, N = 16: rel_l2 {rel_l2(out, ref):.3e}, max {max_rel(out, ref):.3e}; against the plain forward {rel_l2(out, plain):.3e}")
    assert_close(out, ref, TOL_MODEL, TOL_MODEL_MAX, "adapted forward on 16 resampled tokens")
    assert rel_l2(out, plain) > 10 * TOL_MODEL, "the adapter does not act on these weights"
    assert _same(unet.forward(lat, cx, temb, ip_adapter=plus.ip, ip_tokens=tok, ip_scale=0.0), plain)


# ---- 6. the session --------------------------------------------------------------------------------------------------------------------------
def test_session_equals_the_host_driven_loop_bitwise(plus, unet, tsd_mod, gpu_ctx):
    import test_gpu_ipadapter as TI   # the host-driven loop and the session driver of the kind-20 tests: they take any adapter and N
    from oracle import rng
    case = TI.S_CASES[0]              # seeded DDPM
    assert case[0] == "ddpm_seeded"
    B, L = TI.S_B, TI.S_L
    lat = rng.normal(7, 2200, B * 4 * L * L).reshape(B, 4, L, L)
    inp = dict(lat=lat, ctx=rng.normal(7, 2201, B * T * 768).reshape(B, T, 768), uctx=rng.normal(7, 2202, B * T * 768).reshape(B, T, 768),
               hint=None, nz=None, tok=plus.ip.resample(hidden_of(B, 49)),
               utok=plus.ip.resample(hidden_of(B, 48)))   # the unconditional half: any other 16 tokens
    assert inp["tok"].shape == inp["utok"].shape == (B, 16, 768)
    trio = (unet, plus.ip, None)
    with TI.hoist(tsd_mod, gpu_ctx, 1):
        got = TI.session_run(tsd_mod, trio, case, True, inp, dict(scale=TI.S_SCALE))
        plain = TI.session_run(tsd_mod, trio, case, True, inp, None)
    want = TI.host_loop(tsd_mod, gpu_ctx, trio, case, True, inp, lambda i: TI.S_SCALE)
    for i in range(TI.S_STEPS):
        assert np.isfinite(got[i]).all()
        assert _same(got[i], want[i]), (i, float(np.abs(got[i] - want[i]).max()))
    assert rel_l2(got[-1], plain[-1]) > 1e-3
    s = tsd_mod.Session(unet.model, None, B, L, T, cfg=True)
    s.set_schedule(TI.S_NTRAIN, TI.S_STEPS, 0)
    s.upload(lat, inp["ctx"], inp["uctx"], None)
    s.set_ip_adapter(plus.ip, inp["tok"], inp["utok"])
    with pytest.raises(tsd_mod.TsdError) as e:
        s.slots_open()
    assert e.value.code == tsd_mod._lib.TSD_E_STATE
    s.close()


# ---- 7. generate -----------------------------------------------------------------------------------------------------------------------------
def test_generate_from_pixels_equals_generate_from_hidden_states_and_the_session_loop(plus, unet, tsd_mod):
    from oracle import rng
    B, L, STEPS, SEEDS, CFG_SCALE, IP_SCALE = 2, 16, 2, [777, 778], 7.5, 0.8
    enc = tsd_mod.CLIPVision(seed=11)
    try:
        img = (rng.uniform(7, 2300, 3 * 64 * 48, 0.5) + np.float32(0.5)).reshape(3, 64, 48) * np.float32(255.0)
        cx = rng.normal(7, 2301, B * T * 768).reshape(B, T, 768)
        uctx = rng.normal(7, 2302, B * T * 768).reshape(B, T, 768)
        kw = dict(uncond_context=uctx, cfg=True, cfg_scale=CFG_SCALE, inference_steps=STEPS, strength=1.0, L=L, return_latents=True, seeds=SEEDS,
                  ip_adapter=plus.ip, ip_scale=IP_SCALE)
        a = tsd_mod.generate(unet, None, cx, ip_image=img, image_encoder=enc, **kw)
        hid = enc.forward(img, hidden=True)[1]
        uhid = enc.forward(tsd_mod.clip_neutral_image(), hidden=True)[1]
        assert hid.shape == uhid.shape == (257, 1280)
        b = tsd_mod.generate(unet, None, cx, ip_hidden=hid, ip_uncond_hidden=uhid, **kw)
        assert np.isfinite(a).all() and _same(a, b)
        b2 = tsd_mod.generate(unet, None, cx, ip_hidden=hid, image_encoder=enc, **kw)     # the unconditional half computed by generate
        assert _same(a, b2)
        s = tsd_mod.Session(unet.model, None, B, L, T, cfg=True)
        s.set_schedule(1000, STEPS, 0)
        s.upload(np.zeros((B, 4, L, L), np.float32), cx, uctx, None, cfg_scale=CFG_SCALE)
        s.set_seeds(SEEDS)
        s.seed_latents()
        rep = lambda x: np.repeat(x[None], B, axis=0)  # noqa: E731
        s.set_ip_adapter(plus.ip, plus.ip.resample(rep(hid)), plus.ip.resample(rep(uhid)), scale=IP_SCALE)
        for i in range(STEPS):
            s.step(i)
        want = s.latents()
        s.close()
        assert _same(a, want)
        kw_plain = {k: v for k, v in kw.items() if not k.startswith("ip_")}
        assert not _same(a, tsd_mod.generate(unet, None, cx, **kw_plain))
        with pytest.raises(ValueError, match="plus adapter reads"):
            tsd_mod.generate(unet, None, cx, ip_image_embeds=np.zeros(1024, np.float32), **kw)
    finally:
        enc.model.close()


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    import tsd
    tsd.set_strict(True)
    _ip = tsd.IPAdapter(variant=KIND, params=R.draw_params(DRAW_SEED))
    print(json.dumps({"name": "resample", "digests": jitter_digests(_ip, int(sys.argv[2]))}), flush=True)
    _ip.model.close()
