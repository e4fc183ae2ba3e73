"""GPU: the IP-Adapter.  (1) k_ip_attn_add (csrc/kernels_ipattn.hip) held to the fp64 reference of tests/ipadapter_ref.py element-wise
through tsd_debug_ip_attn_run: d = 40 / 80 / 160 with 8 heads, N = 1 / 4 / 5 / 16 tokens, S = 4 / 16 / 48 / 80 queries, B = 3 with scales
(0, 1, 0.37) and pitch gaps on q and o; a negative scale; scores that span the fp16 exponent range of p; the scale-0 sample's NaN payloads;
finite garbage in the pad keys; batch position, run-to-run and the jitter build's bits; the refusals.  (2) the model level on kinds 5 and 6:
the projection, the adapted forward against the numpy restatement, against the plain forward, at scale 0, with ip = NULL (same launch
list), with a ControlNet, the refusals.  (3) the session: bitwise the host-driven loop of tsd_diffusion_forward_ip_hw plus the update
entries, `generate`, the slot refusals.

Worst error / bound on an MI355X: sweep 0.998 / 0.999 / 0.999 at d = 40 / 80 / 160 (the final fp16 rounding is most of the bound: a worst case near
1 is a half-ulp rounding of the result); negative scales 0.892; scores over 22 / 20 units, where the smallest p underflow, 0.890 / 0.936.
No guard or pitch-gap element was written; the jitter build gave the shipped digest in 8 of 8 repeats of all four cases."""
import ctypes as C
import contextlib
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

import controlnet_ref as CR
import ipadapter_ref as R
import replay
from oracle import models, ops, rng, spec
from util import TOL_MODEL, TOL_MODEL_MAX, assert_close, rel_l2

pytestmark = pytest.mark.gpu
SCALES3 = [0.0, 1.0, 0.37]
NS = ((1, 4), (4, 16), (5, 48), (16, 80), (4, 4), (1, 80), (16, 4), (5, 16), (4, 48), (4, 80), (16, 16), (1, 48), (5, 4), (1, 16), (16, 48), (5, 80))
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
JITTER_REPEATS = 8


@pytest.fixture(scope="module")
def ctx(gpu_ctx, tsd_mod):
    c = tsd_mod.Context(gpu_ctx.device)
    yield c
    c.close()


def run(ctx, d, ops_):
    rc, outs, info = replay.run("tsd_debug_ip_attn_run", ctx, d, ops_, R.PO, R.INPUTS, ("O",), R.dtype_of, R.extents)
    return rc, outs["O"], int(info[R.PI["CHANGED"]])


def verify(ctx, name, d, ops_):
    rc, out, changed = run(ctx, d, ops_)
    assert rc == 0, f"{name}: status {rc}: {replay.lib().tsd_last_error().decode()}"
    assert changed == 0, f"{name}: {changed} guard / pitch-gap elements written"
    replay.assert_gaps_hold_fill(out, R.o_index(d), f"{name}: O")
    fails, ratio = R.check(d, ops_, out)
    assert not fails, f"{name}: " + "; ".join(fails)
    # a sample at scale 0 is not touched
    s = ops_["S"]
    y, o = R.unpack_output(d, out), R.unpack(d, ops_)[3]
    for b in np.nonzero(s == 0)[0]:
        assert np.array_equal(y[b].view(np.uint16), o[b].view(np.uint16)), f"{name}: the scale-0 sample {b} was written"
    return out, ratio


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", (40, 80, 160))
def test_kernel_matches_the_fp64_reference_over_the_sweep(ctx, hd):
    worst = 0.0
    for N, S in NS:
        d = R.desc(3, 8, hd, S, N)
        ops_ = R.make_inputs(d, seed=1000 + hd + 7 * N + S, scales=SCALES3)
        assert R.well_conditioned(d, ops_)
        _, ratio = verify(ctx, f"d{hd} N{N} S{S}", d, ops_)
        worst = max(worst, ratio)
    print(f"[ipattn] d = {hd}: worst error / bound over {len(NS)} shapes {worst:.3f}")


def test_negative_scale_and_scores_over_the_fp16_exponent_range_of_p(ctx):
    d = R.desc(3, 8, 80, 48, 5)
    _, r0 = verify(ctx, "negative", d, R.make_inputs(d, seed=3, scales=[-0.8, 1.0, -2.0]))
    d = R.desc(2, 8, 40, 16, 16)
    ops_ = R.make_inputs(d, seed=5, scales=[1.0, -0.8], span=22.0)
    assert not R.well_conditioned(d, ops_)
    _, r1 = verify(ctx, "underflow", d, ops_)
    d = R.desc(1, 8, 160, 80, 16)
    _, r2 = verify(ctx, "underflow160", d, R.make_inputs(d, seed=6, span=20.0))
    print(f"[ipattn] negative scales {r0:.3f}; scores over 22 / 20 units (p underflows) {r1:.3f} {r2:.3f}")


def test_scale_zero_sample_keeps_its_nan_payloads(ctx):
    d = R.desc(3, 8, 40, 48, 4)
    ops_ = R.make_inputs(d, seed=11, scales=SCALES3)
    idx0 = R.o_index(d)[0]
    payload = (0x7E01 + (np.arange(idx0.size) % 251)).astype(np.uint16).reshape(idx0.shape)   # quiet NaNs with distinct payloads
    ops_["OIN"].view(np.uint16)[idx0] = payload
    rc, out, changed = run(ctx, d, ops_)
    assert rc == 0 and changed == 0
    assert np.array_equal(out.view(np.uint16)[idx0], payload), "the scale-0 sample was rewritten"
    y = R.unpack_output(d, out)
    assert np.isfinite(y[1:].astype(np.float32)).all()
    clean = R.make_inputs(d, seed=11, scales=SCALES3)
    rc, out2, _ = run(ctx, d, clean)
    assert np.array_equal(R.unpack_output(d, out2)[1:].view(np.uint16), y[1:].view(np.uint16))   # nothing of sample 0 reached the others


@pytest.mark.parametrize("hd,N", [(40, 1), (80, 4), (160, 5)])
def test_finite_values_in_the_pad_keys_change_no_bit(ctx, hd, N):
    d = R.desc(2, 8, hd, 16, N)
    z = R.make_inputs(d, seed=21, pad=0.0)
    f = R.make_inputs(d, seed=21, pad=60000.0)
    assert not np.array_equal(z["K"].view(np.uint16), f["K"].view(np.uint16)) and not np.array_equal(z["VT"].view(np.uint16), f["VT"].view(np.uint16))
    y0, _ = verify(ctx, "pad0", d, z)
    rc, y1, changed = run(ctx, d, f)
    assert rc == 0 and changed == 0
    assert np.array_equal(y0.view(np.uint16), y1.view(np.uint16)), "rows N .. 15 of K_ip / V_ip^T reached the output"


def test_batch_position_and_run_to_run_are_bitwise(ctx):
    for hd, N, S in ((40, 4, 80), (160, 5, 48)):
        d3 = R.desc(3, 8, hd, S, N)
        ops3 = R.make_inputs(d3, seed=31, scales=[1.0, 1.0, 1.0])
        y3, _ = verify(ctx, "b3", d3, ops3)
        y3b, _ = verify(ctx, "b3/again", d3, ops3)
        assert np.array_equal(y3.view(np.uint16), y3b.view(np.uint16))
        q, k, vt, o, s = R.unpack(d3, ops3)
        for src in range(3):          # sample `src` alone, and in every position of a batch of 3 beside other samples
            d1 = R.desc(1, 8, hd, S, N)
            y1, _ = verify(ctx, f"b1/{src}", d1, R.pack(d1, q[src:src + 1], k[src:src + 1], vt[src:src + 1], o[src:src + 1], s[src:src + 1]))
            want = R.unpack_output(d3, y3)[src].view(np.uint16)
            assert np.array_equal(R.unpack_output(d1, y1)[0].view(np.uint16), want), (hd, src)
            for pos in range(3):
                order = [(src + j - pos) % 3 for j in range(3)]
                yp, _ = verify(ctx, f"perm/{src}/{pos}", d3, R.pack(d3, q[order], k[order], vt[order], o[order], s[order]))
                assert np.array_equal(R.unpack_output(d3, yp)[pos].view(np.uint16), want), (hd, src, pos)


def test_refusals_leave_the_output_untouched(ctx):
    good = R.desc(1, 8, 40, 16, 4)
    ops_ = R.make_inputs(good, seed=41)
    for name, field, value in (("N=0", "N", 0), ("N=17", "N", 17), ("S%4", "S", 18)):
        d = good.copy()
        d[R.PD[field]] = value
        if field == "S":
            d = R.desc(1, 8, 40, 18, 4)
        o = R.make_inputs(d, seed=41) if field == "S" else ops_
        rc, out, changed = run(ctx, d, o)
        assert rc == -2, f"{name}: status {rc}"   # TSD_E_SHAPE
        assert changed == 0
        assert np.array_equal(out.view(np.uint16), o["OIN"].view(np.uint16)), f"{name}: O was written"
    d64 = R.desc(1, 8, 64, 16, 4)
    rc, out, changed = run(ctx, d64, R.make_inputs(d64, seed=42))
    assert rc == -2 and changed == 0
    # a NULL operand
    dd = np.ascontiguousarray(good, np.int64)
    rcs, ext = replay.size("tsd_debug_ip_attn_run", dd, ctx=ctx.h)
    assert rcs == 0
    ins = (C.c_void_p * R.PO["COUNT"])()
    for s_ in R.INPUTS:
        if s_ != "K":
            ins[R.PO[s_]] = ops_[s_].ctypes.data
    outbuf = np.empty(R.extents(good)["O"], np.float16)
    outp = (C.c_void_p * 1)(outbuf.ctypes.data)
    info = np.zeros(8, np.int64)
    i64p = C.POINTER(C.c_int64)
    rc = replay.lib().tsd_debug_ip_attn_run(ctx.h, dd.ctypes.data_as(i64p), len(dd), ins, outp, ext.ctypes.data_as(i64p), info.ctypes.data_as(i64p))
    assert rc == -1   # TSD_E_ARG


def test_op_entry_agrees_with_the_replay_entry(ctx, tsd_mod):
    d = R.desc(2, 8, 80, 48, 4, gap=0, sgap=0)
    ops_ = R.make_inputs(d, seed=51, scales=[1.0, 0.5])
    y, _ = verify(ctx, "dense", d, ops_)
    q, k, vt, o, s = R.unpack(d, ops_)
    got = tsd_mod.ip_attn_add(q, k, vt, o, s, 8, 4, ctx=ctx)
    assert np.array_equal(got.view(np.uint16), R.unpack_output(d, y).view(np.uint16))
    with pytest.raises(tsd_mod.TsdError) as e:
        tsd_mod.ip_attn_add(q, k, vt, o, s, 8, 0, ctx=ctx)
    assert e.value.code == tsd_mod._lib.TSD_E_SHAPE


JITTER_SHAPES = ((40, 4, 80), (80, 5, 48), (160, 16, 16), (40, 1, 4))


def jitter_cases(c, repeats):
    out = []
    for hd, N, S in JITTER_SHAPES:
        d = R.desc(3, 8, hd, S, N)
        ops_ = R.make_inputs(d, seed=61 + hd, scales=SCALES3)
        digs = []
        for _ in range(repeats):
            rc, y, changed = run(c, d, ops_)
            assert rc == 0 and changed == 0
            digs.append(hashlib.sha256(y.view(np.uint16).tobytes()).hexdigest()[:16])
        out.append((f"d{hd}_N{N}_S{S}", digs))
    return out


def test_jitter_build_reproduces_the_shipped_bits(ctx):
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    here = jitter_cases(ctx, 1)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [r["name"] for r in there] == [n for n, _ in here]
    for (name, mine), theirs in zip(here, there):
        assert len(theirs["digests"]) == JITTER_REPEATS
        assert all(dg == mine[0] for dg in theirs["digests"]), f"{name}: the jitter build gave {len(set(theirs['digests']))} result(s), not the shipped bits"


# ---- 2. the models ------------------------------------------------------------------------------------------------------------------------
SEED, IP_SEED, CN_SEED, T = 1234, 9, 5, 77
VARIANTS = {"reference": ("diffusion_sd15", "controlnet_sd15", False), "torch": ("diffusion_sd15_torch", "controlnet_sd15_torch", True)}
SHAPES = ((16, 16), (16, 32))
IP_SCALES = (1.0, 0.6)
CN_SCALES = (1.0, 0.5)


def _inputs(B, LH, LW, tag):
    lat = rng.normal(7, tag, B * 4 * LH * LW).reshape(B, 4, LH, LW)
    cx = rng.normal(7, tag + 1, B * T * 768).reshape(B, T, 768)
    emb = rng.normal(7, tag + 2, B * 1024).reshape(B, 1024)
    hint = (rng.uniform(7, tag + 3, B * 3 * 64 * LH * LW, 0.5) + np.float32(0.5)).reshape(B, 3, 8 * LH, 8 * LW)
    temb = np.stack([ops.time_embedding(t) for t in (980.0, 20.0, 500.0)[:B]])
    return lat, cx, temb, emb, hint


class World:
    """The UNet of one variant, an init_random adapter and a ControlNet, with the reference of every shape computed once."""

    def __init__(self, tsd_mod, name):
        self.name = name
        self.unet_kind, self.cn_kind, self.tn = VARIANTS[name]
        self.ip = tsd_mod.IPAdapter(seed=IP_SEED)
        self.PI = {n: self.ip.model.get_param(n) for n, *_ in tsd_mod.param_specs("ip_adapter_sd15")}
        self.d = tsd_mod.Diffusion(seed=SEED, variant=self.unet_kind)
        self.PC = CR.draw_params(tsd_mod.param_specs(self.cn_kind), CN_SEED, nonzero=("zero.", "hint.conv8"))
        self.cn = tsd_mod.ControlNet(params=self.PC, variant=self.cn_kind)
        PU = spec.init_params(self.unet_kind, SEED, only_used=not self.tn)
        self.cases = {}
        for i, (LH, LW) in enumerate(SHAPES):
            lat, cx, temb, emb, hint = _inputs(2, LH, LW, 1700 + 10 * i)
            tok = R.project(self.PI, emb)
            ref = []
            for b in range(2):
                with R.adapted(PU, self.PI, tok[b], IP_SCALES[b]):
                    ref.append(CR.diffusion_sd15_controlled(PU, lat[b], cx[b], temb[b], None, 0.0, tn=self.tn))
            case = dict(lat=lat, ctx=cx, temb=temb, emb=emb, hint=hint, tok_ref=tok, ref=np.stack(ref))
            if i == 0:   # adapter and ControlNet together, one shape
                both = []
                for b in range(2):
                    res = CR.controlnet(self.PC, lat[b], cx[b], temb[b], hint[b], tn=self.tn)
                    with R.adapted(PU, self.PI, tok[b], IP_SCALES[b]):
                        both.append(CR.diffusion_sd15_controlled(PU, lat[b], cx[b], temb[b], res, CN_SCALES[b], tn=self.tn))
                case["ref_both"] = np.stack(both)
            self.cases[(LH, LW)] = case
        del PU

    def close(self):
        for m in (self.ip, self.d, self.cn):
            m.model.close()


@pytest.fixture(scope="module", params=list(VARIANTS))
def world(request, gpu_ctx, tsd_mod):
    w = World(tsd_mod, request.param)
    yield w
    w.close()


def test_projection_matches_numpy(world):
    c = world.cases[SHAPES[0]]
    tok = world.ip.project(c["emb"])
    assert tok.shape == (2, 4, 768)
    assert_close(tok, c["tok_ref"], TOL_MODEL, TOL_MODEL_MAX, "image projection")
    np.testing.assert_array_equal(world.ip.project(c["emb"][1]), tok[1])
    assert np.array_equal(tok.astype(np.float16).astype(np.float32), tok)   # every token value is an fp16


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_adapted_forward_matches_the_restatement_and_differs_from_the_plain_forward(world, shape, gpu_ctx):
    c = world.cases[shape]
    tok = world.ip.project(c["emb"])
    out = world.d.forward(c["lat"], c["ctx"], c["temb"], ip_adapter=world.ip, ip_tokens=tok, ip_scale=IP_SCALES)
    assert_close(out, c["ref"], TOL_MODEL, TOL_MODEL_MAX, f"{world.name} {shape} adapted forward")
    plain = world.d.forward(c["lat"], c["ctx"], c["temb"])
    acts = rel_l2(out, plain)
    print(f"[ip] {world.name} {shape}: rel_l2 against the plain forward {acts:.3e}")
    assert acts > 10 * TOL_MODEL, "the adapter does not act on these weights"
    np.testing.assert_array_equal(world.d.forward(c["lat"], c["ctx"], c["temb"], ip_adapter=world.ip, ip_tokens=tok, ip_scale=IP_SCALES), out)
    # scale 0 for all samples is the plain forward
    np.testing.assert_array_equal(world.d.forward(c["lat"], c["ctx"], c["temb"], ip_adapter=world.ip, ip_tokens=tok, ip_scale=0.0), plain)
    # per-sample scales: a sample's result does not depend on the other sample's scale
    mixed = world.d.forward(c["lat"], c["ctx"], c["temb"], ip_adapter=world.ip, ip_tokens=tok, ip_scale=(IP_SCALES[0], 0.0))
    np.testing.assert_array_equal(mixed[0], out[0])
    assert rel_l2(mixed[1], plain[1]) < TOL_MODEL


def _records(gpu_ctx, fn):
    gpu_ctx.profile_begin()
    try:
        fn()
        return [r[:5] for r in gpu_ctx.profile_records()]
    finally:
        gpu_ctx.profile_end()


def test_no_adapter_records_the_plain_launch_list(world, tsd_mod, gpu_ctx):
    from tsd._lib import f32, lib, ptr
    c = world.cases[SHAPES[0]]
    lat, cx, temb = f32(c["lat"]), f32(c["ctx"]), f32(c["temb"])
    out = np.empty_like(lat)

    def null_ip():
        rc = lib().tsd_diffusion_forward_ip_hw(world.d.model.h, None, None, 0, None, None, None, None, ptr(lat), ptr(cx), ptr(temb), 2, 16, 16, T, ptr(out))
        assert rc == 0
    plain_list = _records(gpu_ctx, lambda: world.d.forward(lat, cx, temb))
    assert plain_list and _records(gpu_ctx, null_ip) == plain_list
    np.testing.assert_array_equal(out, world.d.forward(lat, cx, temb))
    tok = world.ip.project(c["emb"])
    with_ip = _records(gpu_ctx, lambda: world.d.forward(lat, cx, temb, ip_adapter=world.ip, ip_tokens=tok))
    n_attn = lambda recs: sum(1 for r in recs if r[0] == "attn")   # noqa: E731
    assert n_attn(with_ip) >= n_attn(plain_list) + 16 or len(with_ip) > len(plain_list)


def test_adapter_and_controlnet_compose(world):
    c = world.cases[SHAPES[0]]
    tok = world.ip.project(c["emb"])
    out = world.d.forward(c["lat"], c["ctx"], c["temb"], control=world.cn, hint=c["hint"], control_scale=CN_SCALES, ip_adapter=world.ip,
                          ip_tokens=tok, ip_scale=IP_SCALES)
    assert_close(out, c["ref_both"], TOL_MODEL, TOL_MODEL_MAX, f"{world.name} adapter + ControlNet")
    only_cn = world.d.forward(c["lat"], c["ctx"], c["temb"], control=world.cn, hint=c["hint"], control_scale=CN_SCALES)
    assert rel_l2(out, only_cn) > 10 * TOL_MODEL
    np.testing.assert_array_equal(world.d.forward(c["lat"], c["ctx"], c["temb"], control=world.cn, hint=c["hint"], control_scale=CN_SCALES,
                                                  ip_adapter=world.ip, ip_tokens=tok, ip_scale=0.0), only_cn)


def test_forward_refusals(world, tsd_mod, gpu_ctx):
    E = tsd_mod._lib
    c = world.cases[SHAPES[0]]
    tok = world.ip.project(c["emb"])
    args = (c["lat"], c["ctx"], c["temb"])

    def code(fn):
        with pytest.raises(tsd_mod.TsdError) as e:
            fn()
        return e.value.code
    tiny = tsd_mod.Diffusion(seed=SEED)
    assert code(lambda: tiny.forward(*args, ip_adapter=world.ip, ip_tokens=tok)) == E.TSD_E_ARG              # the Tiny-SD graph
    tiny.model.close()
    assert code(lambda: world.d.forward(*args, ip_adapter=world.d, ip_tokens=tok)) == E.TSD_E_ARG            # `ip` is no adapter
    assert code(lambda: tsd_mod.Diffusion.forward(world.cn, *args, ip_adapter=world.ip, ip_tokens=tok)) == E.TSD_E_ARG   # a ControlNet as the UNet
    assert code(lambda: world.d.forward(*args, ip_adapter=world.ip, ip_tokens=tok, ip_scale=float("nan"))) == E.TSD_E_ARG
    with pytest.raises(ValueError):
        world.d.forward(*args, ip_adapter=world.ip, ip_tokens=np.zeros((2, 17, 768), np.float32))
    with pytest.raises(ValueError):
        world.d.forward(*args, ip_tokens=tok)
    ctx2 = tsd_mod.Context(gpu_ctx.device)
    far = tsd_mod.IPAdapter(seed=1, ctx=ctx2)
    assert code(lambda: world.d.forward(*args, ip_adapter=far, ip_tokens=tok)) == E.TSD_E_ARG                # another context
    far.model.close(); ctx2.close()
    if world.tn:   # the SD-2.x UNet reads a 1024-wide context: an SD-1.x adapter is refused
        sd2 = tsd_mod.Diffusion(seed=SEED, variant="diffusion_sd2")
        cx2 = rng.normal(7, 77, 2 * T * 1024).reshape(2, T, 1024)
        assert code(lambda: sd2.forward(c["lat"], cx2, c["temb"], ip_adapter=world.ip, ip_tokens=tok)) == E.TSD_E_ARG
        sd2.model.close()


# ---- 3. the session -----------------------------------------------------------------------------------------------------------------------
S_L, S_B, S_STEPS, S_NTRAIN, S_SCALE, S_CFG_SCALE = 16, 2, 3, 1000, 0.8, 7.5
S_KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}
S_SPACINGS = {"leading": 0, "trailing": 1}
S_CASES = [("ddpm_seeded", "epsilon", False, ("ddpm", 0.0, "leading"), "seeded"), ("dpmpp_2m", "epsilon", False, ("dpmpp_2m", 0.0, "trailing"), None),
           ("vpred", "v", True, ("ddpm", 0.0, "trailing"), "upload")]
S_SEEDS = [777, 778]


@contextlib.contextmanager
def hoist(tsd_mod, gpu_ctx, on):
    lib = tsd_mod._lib.lib()
    prev = lib.tsd_debug_set_session_hoist(gpu_ctx.h, int(on))
    try:
        yield
    finally:
        lib.tsd_debug_set_session_hoist(gpu_ctx.h, prev)


@pytest.fixture(scope="module")
def trio(gpu_ctx, tsd_mod):
    """The reference-kind UNet, an adapter and a ControlNet (no numpy reference: everything is held to the device's own forward)."""
    d = tsd_mod.Diffusion(seed=SEED, variant="diffusion_sd15")
    ip = tsd_mod.IPAdapter(seed=IP_SEED)
    cn = tsd_mod.ControlNet(params=CR.draw_params(tsd_mod.param_specs("controlnet_sd15"), CN_SEED, nonzero=("zero.", "hint.conv8")), variant="controlnet_sd15")
    yield d, ip, cn
    for m in (d, ip, cn):
        m.model.close()


def _s_inputs(ip, tag):
    lat, cx, _, emb, hint = _inputs(S_B, S_L, S_L, tag)
    uctx = rng.normal(7, tag + 5, S_B * T * 768).reshape(S_B, T, 768)
    nz = rng.normal(7, tag + 6, S_STEPS * lat.size).reshape((S_STEPS,) + lat.shape)
    return dict(lat=lat, ctx=cx, uctx=uctx, hint=hint, nz=nz, tok=ip.project(emb), utok=ip.project(np.zeros_like(emb)))


def _coeffs(tsd_mod, sampler, i, have_history, pred, ztsnr):
    kind, eta, spacing = sampler
    out = (C.c_double * 8)()
    rc = tsd_mod._lib.lib().tsd_sampler_coeffs_ex(S_KINDS[kind], float(eta), S_SPACINGS[spacing], S_NTRAIN, S_STEPS, 0, i, int(have_history),
                                                  tsd_mod._lib.PREDICTION_TYPES[pred], int(ztsnr), out)
    assert rc == 0, tsd_mod._lib.last_error()
    return np.array(out[:], dtype=np.float64)


def _eps_step(tsd_mod, gpu_ctx, x, e_c, e_u, scale, hist, noise, c, keep_hist):
    from tsd._lib import check, f32, ptr
    x, e_c = f32(x), f32(e_c)
    e_u = f32(e_u) if e_u is not None else None
    out, h = np.empty_like(x), (np.empty_like(x) if keep_hist else None)
    check(tsd_mod._lib.lib().tsd_sampler_step_f32(gpu_ctx.h, ptr(x), ptr(e_c), ptr(e_u), float(scale), ptr(f32(hist)) if hist is not None else None,
                                                  ptr(f32(noise)) if noise is not None else None, x.size, ptr(np.ascontiguousarray(c, dtype=np.float32)),
                                                  ptr(out), ptr(h)))
    return out, h


def host_forward(tsd_mod, d, ip, cn, x, inp, cfg, t, ip_scale, cn_scale):
    """The step's forward from the host at the UNet's batch (tsd_diffusion_forward_ip_hw): -> (cond, uncond or None)."""
    xx = np.concatenate([x, x]) if cfg else x
    cc = np.concatenate([inp["ctx"], inp["uctx"]]) if cfg else inp["ctx"]
    temb = np.repeat(tsd_mod.get_time_embedding(float(t)).reshape(1, 320), xx.shape[0], axis=0)
    kw = {}
    if ip_scale is not None:
        kw.update(ip_adapter=ip, ip_tokens=np.concatenate([inp["tok"], inp["utok"]]) if cfg else inp["tok"], ip_scale=ip_scale)
    if cn_scale is not None:
        kw.update(control=cn, hint=np.concatenate([inp["hint"], inp["hint"]]) if cfg else inp["hint"], control_scale=cn_scale)
    e = d.forward(xx, cc, temb, **kw)
    return (e[:S_B], e[S_B:]) if cfg else (e, None)


def host_loop(tsd_mod, gpu_ctx, trio, case, cfg, inp, ip_of_step, cn_scale=None, extras=None):
    """[latents after step i] of the host-driven loop; ip_of_step(i) -> the adapter's scale at step i, or None."""
    d, ip, cn = trio
    _, pred, ztsnr, sampler, noise_kind = case
    kind = sampler[0]
    x, hist, outs = inp["lat"], None, []
    multistep = kind == "dpmpp_2m"
    for i in range(S_STEPS):
        cd = _coeffs(tsd_mod, sampler, i, hist is not None, pred, ztsnr)
        e_c, e_u = host_forward(tsd_mod, d, ip, cn, x, inp, cfg, int(cd[0]), ip_of_step(i), cn_scale)
        if extras and extras.get("phi"):
            e_c, e_u, _ = tsd_mod.cfg_rescale(e_c, e_u, S_CFG_SCALE, extras["phi"], ctx=gpu_ctx)
        if noise_kind == "seeded":
            noise = np.stack([tsd_mod.normal_fill(sd, 16 + i, x[0].size, ctx=gpu_ctx).reshape(x[0].shape) for sd in S_SEEDS])
        else:
            noise = inp["nz"][i] if noise_kind == "upload" else None
        c = cd[2:].astype(np.float32)
        if pred == "v":
            x, h = tsd_mod.sampler_step_v(x, e_c, e_u, S_CFG_SCALE, hist, noise if (noise is not None and c[5] != 0) else None, c, multistep, ctx=gpu_ctx)
        elif kind == "ddpm":
            x, h = tsd_mod.ddpm_step(x, e_c, e_u, S_CFG_SCALE, noise, i, S_STEPS, S_NTRAIN, 0, sampler[2], ctx=gpu_ctx), None
        else:
            x, h = _eps_step(tsd_mod, gpu_ctx, x, e_c, e_u, S_CFG_SCALE, hist, noise if c[5] != 0 else None, c, multistep)
        hist = h if multistep else None
        if extras and extras.get("mask") is not None:
            nxt = _coeffs(tsd_mod, sampler, i + 1, False, pred, ztsnr) if i + 1 < S_STEPS else None
            a_prev, s_prev = (np.float32(nxt[2]), np.float32(nxt[3])) if nxt is not None else (np.float32(1.0), np.float32(0.0))
            x = tsd_mod.inpaint_blend(x, extras["mask"], extras["known"], extras["ip_noise"], a_prev, s_prev, ctx=gpu_ctx)
        outs.append(x)
    return outs


def _open(tsd_mod, d, cfg, case):
    _, pred, ztsnr, sampler, _ = case
    s = tsd_mod.Session(d.model, None, S_B, S_L, T, cfg=cfg)
    s.set_prediction(pred, ztsnr)
    s.set_sampler(*sampler)
    s.set_schedule(S_NTRAIN, S_STEPS, 0)
    return s


def _start(s, case, cfg, inp, extras=None):
    s.upload(inp["lat"], inp["ctx"], inp["uctx"] if cfg else None, inp["nz"] if case[4] == "upload" else None, cfg_scale=S_CFG_SCALE)
    if case[4] == "seeded":
        s.set_seeds(S_SEEDS)
    if extras and extras.get("mask") is not None:
        s.set_inpaint(extras["mask"], extras["known"], extras["ip_noise"])
    if extras and extras.get("phi"):
        s.set_guidance_rescale(extras["phi"])


def session_run(tsd_mod, trio, case, cfg, inp, adapter, control=None, extras=None, off_after=None):
    """[latents after step i] of a session; adapter: None, or the keywords of set_ip_adapter; off_after: set_ip_adapter(None) after that step."""
    d, ip, cn = trio
    s = _open(tsd_mod, d, cfg, case)
    _start(s, case, cfg, inp, extras)
    if control is not None:
        s.set_control(cn, inp["hint"], **control)
    if adapter is not None:
        s.set_ip_adapter(ip, inp["tok"], inp["utok"] if cfg else None, **adapter)
        assert s.ip_adapter_active
    outs = []
    for i in range(S_STEPS):
        s.step(i)
        outs.append(s.latents())
        if off_after == i:
            s.set_ip_adapter(None)
            assert not s.ip_adapter_active
    s.close()
    return outs


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("on", [1, 0], ids=["hoist", "nohoist"])
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("case", S_CASES, ids=[c[0] for c in S_CASES])
def test_session_with_an_adapter_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod, trio, case, cfg, on):
    inp = _s_inputs(trio[1], 1900)
    with hoist(tsd_mod, gpu_ctx, on):
        got = session_run(tsd_mod, trio, case, cfg, inp, dict(scale=S_SCALE))
        plain = session_run(tsd_mod, trio, case, cfg, inp, None)
    want = host_loop(tsd_mod, gpu_ctx, trio, case, cfg, inp, lambda i: S_SCALE)
    for i in range(S_STEPS):
        assert np.isfinite(got[i]).all()
        assert _same(got[i], want[i]), (case[0], cfg, on, i, float(np.abs(got[i] - want[i]).max()))
    assert rel_l2(got[-1], plain[-1]) > 1e-3   # the adapter acts on the session's latents


def test_session_window_turning_the_adapter_off_and_an_upload(gpu_ctx, tsd_mod, trio):
    d, ip, cn = trio
    case, inp = S_CASES[0], _s_inputs(ip, 1910)
    plain = session_run(tsd_mod, trio, case, True, inp, None)
    full = session_run(tsd_mod, trio, case, True, inp, dict(scale=S_SCALE))
    win = session_run(tsd_mod, trio, case, True, inp, dict(scale=S_SCALE, first_step=1, last_step=1))
    want = host_loop(tsd_mod, gpu_ctx, trio, case, True, inp, lambda i: S_SCALE if i == 1 else None)
    assert _same(win[0], plain[0]) and all(_same(g, w) for g, w in zip(win, want)) and not _same(win[1], plain[1])
    off = session_run(tsd_mod, trio, case, True, inp, dict(scale=S_SCALE), off_after=0)   # set_ip_adapter(NULL) mid-run
    want = host_loop(tsd_mod, gpu_ctx, trio, case, True, inp, lambda i: S_SCALE if i == 0 else None)
    assert _same(off[0], full[0]) and all(_same(g, w) for g, w in zip(off, want))
    zero = session_run(tsd_mod, trio, case, True, inp, dict(scale=0.0))                    # scale 0: the plain session
    assert all(_same(g, w) for g, w in zip(zero, plain))
    # the adapter outlives an upload() and upload() rebuilds nothing of it
    s = _open(tsd_mod, d, True, case)
    _start(s, case, True, inp)
    s.set_ip_adapter(ip, inp["tok"], inp["utok"], scale=S_SCALE)
    _start(s, case, True, inp)
    assert s.ip_adapter_active
    for i in range(S_STEPS):
        s.step(i)
        assert _same(s.latents(), full[i])
    s.close()


def test_session_controlnet_inpainting_guidance_rescale_and_adapter_in_one_run(gpu_ctx, tsd_mod, trio):
    case = ("ddpm_upload", "epsilon", False, ("ddpm", 0.0, "leading"), "upload")
    inp = _s_inputs(trio[1], 1920)
    cell = np.arange(S_L * S_L).reshape(1, S_L, S_L)
    mask = np.repeat(np.where(cell % 13 < 4, 0.0, np.where(cell % 13 > 9, 1.0, (cell % 13) / 16.0)).astype(np.float32), S_B, axis=0)
    n = inp["lat"].size
    extras = dict(mask=mask, known=rng.normal(7, 1925, n).reshape(inp["lat"].shape), ip_noise=rng.normal(7, 1926, n).reshape(inp["lat"].shape), phi=0.7)
    got = session_run(tsd_mod, trio, case, True, inp, dict(scale=S_SCALE), control=dict(scale=0.7), extras=extras)
    want = host_loop(tsd_mod, gpu_ctx, trio, case, True, inp, lambda i: S_SCALE, cn_scale=[0.7] * (2 * S_B), extras=extras)
    for i in range(S_STEPS):
        assert _same(got[i], want[i]), (i, float(np.abs(got[i] - want[i]).max()))
    bare = session_run(tsd_mod, trio, case, True, inp, None, control=dict(scale=0.7), extras=extras)
    assert not _same(got[-1], bare[-1])


def test_generate_with_an_adapter_is_the_session_loop(gpu_ctx, tsd_mod, trio):
    d, ip, cn = trio
    lat, cx, _, emb, _ = _inputs(S_B, S_L, S_L, 1940)
    uctx = rng.normal(7, 1945, S_B * T * 768).reshape(S_B, T, 768)
    kw = dict(uncond_context=uctx, cfg=True, cfg_scale=S_CFG_SCALE, inference_steps=4, strength=1.0, L=S_L, return_latents=True, seeds=S_SEEDS)
    out = tsd_mod.generate(d, None, cx, ip_adapter=ip, ip_image_embeds=emb, ip_scale=S_SCALE, ip_start=0.25, ip_end=0.75, **kw)
    s = tsd_mod.Session(d.model, None, S_B, S_L, T, cfg=True)
    s.set_schedule(S_NTRAIN, 4, 0)
    s.upload(np.zeros_like(lat), cx, uctx, None, cfg_scale=S_CFG_SCALE)
    s.set_seeds(S_SEEDS)
    s.seed_latents()
    s.set_ip_adapter(ip, ip.project(emb), ip.project(np.zeros_like(emb)), scale=S_SCALE, first_step=1, last_step=2)
    for i in range(4):
        s.step(i)
    want = s.latents()
    s.close()
    assert _same(out, want)
    assert not _same(out, tsd_mod.generate(d, None, cx, **kw))
    with pytest.raises(ValueError):
        tsd_mod.generate(d, None, cx, ip_adapter=ip, **kw)


def test_session_refusals(gpu_ctx, tsd_mod, trio):
    d, ip, cn = trio
    E = tsd_mod._lib
    inp = _s_inputs(ip, 1930)

    def code(fn):
        with pytest.raises(tsd_mod.TsdError) as e:
            fn()
        return e.value.code
    s = tsd_mod.Session(d.model, None, S_B, S_L, T, cfg=False)
    s.set_schedule(S_NTRAIN, S_STEPS, 0)
    assert code(lambda: s.set_ip_adapter(ip, inp["tok"])) == E.TSD_E_STATE                       # before upload()
    s.upload(inp["lat"], inp["ctx"], None, None)
    assert code(lambda: s.set_ip_adapter(d, inp["tok"])) == E.TSD_E_ARG                          # no adapter
    assert code(lambda: s.set_ip_adapter(ip, inp["tok"], scale=float("inf"))) == E.TSD_E_ARG
    assert code(lambda: s.set_ip_adapter(ip, inp["tok"], first_step=2, last_step=1)) == E.TSD_E_ARG
    with pytest.raises(ValueError):
        s.set_ip_adapter(ip, np.zeros((S_B, 17, 768), np.float32))
    assert not s.ip_adapter_active
    s.set_ip_adapter(ip, inp["tok"])
    assert code(s.slots_open) == E.TSD_E_STATE                                                   # slots on a session with an adapter
    s.set_ip_adapter(None)
    s.slots_open()
    assert code(lambda: s.set_ip_adapter(ip, inp["tok"])) == E.TSD_E_STATE                       # an adapter on a slot session
    s.close()
    c = tsd_mod.Session(d.model, None, S_B, S_L, T, cfg=True)
    c.set_schedule(S_NTRAIN, S_STEPS, 0)
    c.upload(inp["lat"], inp["ctx"], inp["uctx"], None)
    with pytest.raises(ValueError):                                                               # CFG needs the uncond tokens
        c.set_ip_adapter(ip, inp["tok"])
    from tsd._lib import f32, ptr
    tok = f32(inp["tok"])
    assert tsd_mod._lib.lib().tsd_session_set_ip_adapter(c.h, ip.model.h, ptr(tok), None, 4, 1.0, 0, -1) == E.TSD_E_ARG
    c.close()
    tiny = tsd_mod.Diffusion(seed=SEED)
    t = tsd_mod.Session(tiny.model, None, S_B, S_L, T, cfg=False)
    t.set_schedule(S_NTRAIN, S_STEPS, 0)
    t.upload(inp["lat"], inp["ctx"], None, None)
    assert code(lambda: t.set_ip_adapter(ip, inp["tok"])) == E.TSD_E_ARG                         # the Tiny-SD graph
    t.close(); tiny.model.close()


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    import tsd
    tsd.set_strict(True)
    _c = tsd.Context(0)
    for _name, _digests in jitter_cases(_c, int(sys.argv[2])):
        print(json.dumps({"name": _name, "digests": _digests}), flush=True)
    _c.close()
