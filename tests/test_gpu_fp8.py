"""GPU: the FP8 feed-forward (csrc/kernels_fp8.hip, `tsd_model_set_ff_fp8`) against tests/fp8_ref.py: the quantiser bit for bit, the e4m3
GEMM element-wise under the derived bound, and the model option against the numpy restatement with the two feed-forward linears replaced
by the fake-quant linear.  Run as a program (`jitter-child <repeats>`) it prints the launches' digests on whatever library TSD_LIB names."""
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

import fp8_ref as R
from oracle import rng
from util import TOL_MODEL, rel_l2

pytestmark = pytest.mark.gpu
JITTER_REPEATS = 8
JITTER_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stable-diffusion.mojo_amd", "lib", "libtsd_jitter.so")
QUANT_SHAPES = ((1, 128, 128), (3, 320, 320), (17, 640, 648), (5, 5120, 5120))
# (M, N, K, epilogue): one instruction (pins the lane mapping); one row; K pad and partial tiles both ways; ten K steps through both LDS
# buffers with odd tile counts; the first feed-forward linear's shape with GEGLU
GEMM_CASES = ((16, 16, 128, "none"), (1, 16, 128, "bias"), (130, 144, 320, "bias_res"), (130, 144, 320, "none"), (257, 272, 1280, "bias_res"),
              (64, 2560, 320, "geglu"))


def quant_input(M, K, ld, seed=11):
    """Normal rows of magnitudes 2^-6 .. 2^4, the gap K .. ld NaN (never read), and by row: 0 amax = 448 with elements on e4m3 midpoints
    (17, 19 and k 2^-10 in the subnormal range), 1 all zero, 2 holding 65504, 3 fp16 subnormals, 4 holding an inf."""
    x = (rng.normal(seed, M * K, M * ld).reshape(M, ld) * 2.0 ** (np.arange(M) % 11 - 6)[:, None]).astype(np.float16)
    x[:, K:] = np.nan
    ties = np.array([448, 17, 19, -17, -19, 25, 27] + [k * 2.0 ** -10 for k in range(1, 18)], np.float16)
    x[0, :K] = np.resize(ties, K)
    for row, fill in ((1, lambda r: 0 * r), (2, lambda r: np.where(np.arange(K) == K // 2, 65504, r)),
                      (3, lambda r: ((np.arange(K) % 1024) * 2.0 ** -24).astype(np.float16)), (4, lambda r: np.where(np.arange(K) == K - 1, np.inf, r))):
        if row < M:
            x[row, :K] = fill(x[row, :K])
    return x


@pytest.mark.parametrize("shape", QUANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantiser_is_the_specification_bit_for_bit(gpu_ctx, tsd_mod, shape):
    M, K, ld = shape
    x = quant_input(M, K, ld)
    want_q, want_s = R.quant_rows(x, K)
    Kp = want_q.shape[1]
    q, s = np.full(M * Kp + 64, 0xA5, np.uint8), np.full(M + 16, -7.0, np.float32)   # guard bands behind both outputs
    assert tsd_mod._lib.lib().tsd_quant_rows_e4m3(gpu_ctx.h, x.ctypes.data, M, K, ld, q.ctypes.data, tsd_mod._lib.ptr(s)) == 0
    assert np.array_equal(q[:M * Kp].reshape(M, Kp), want_q) and not q[:M * Kp].reshape(M, Kp)[:, K:].any()
    nan = np.isnan(want_s)
    assert np.array_equal(np.isnan(s[:M]), nan) and np.array_equal(s[:M][~nan].view(np.uint32), want_s[~nan].view(np.uint32))
    assert (q[M * Kp:] == 0xA5).all() and (s[M:] == -7.0).all()
    assert (M <= 4) == (not np.isnan(s[:M]).any())   # the row with an inf, and only it, has a NaN scale


def gemm_case(M, N, K, epi, seed=23):
    """e4m3 bytes of quantised normal draws; row scales 2^-10 .. 2^6 and channel scales that keep the result inside fp16."""
    a8, _ = R.quant_rows(rng.normal(seed, 1, M * K).reshape(M, K).astype(np.float16))
    w8, _ = R.quant_rows(rng.normal(seed, 2, N * K).reshape(N, K).astype(np.float16))
    sa = (2.0 ** (np.arange(M) % 17 - 10)).astype(np.float32)
    sw = (2.0 ** (np.arange(N) % 5 - (24 if epi == "geglu" else 16))).astype(np.float32)
    bias = None if epi == "none" else (rng.normal(seed, 3, N) * 4).astype(np.float32)
    res = (rng.normal(seed, 4, M * (N + 8)).reshape(M, N + 8) * 4).astype(np.float16) if epi == "bias_res" else None   # pitch N + 8
    return a8, sa, w8, sw, bias, res, R.EPI_GEGLU if epi == "geglu" else R.EPI_NONE


def run_gemm(tsd_mod, case):
    a8, sa, w8, sw, bias, res, epi = case
    width = w8.shape[0] // 2 if epi else w8.shape[0]
    out = np.full((a8.shape[0], width + 4), 123.0, np.float16)   # output pitch width + 4: the gap must come back as it went
    return tsd_mod.fp8_gemm(a8, sa, w8, sw, bias=bias, residual=res, epi=epi, out=out), width


@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gemm_is_under_the_derived_bound_elementwise(gpu_ctx, tsd_mod, case):
    ops = gemm_case(*case)
    out, width = run_gemm(tsd_mod, ops)
    ref, bound = R.gemm(ops[0], ops[1], ops[2], ops[3], ops[4], None if ops[5] is None else ops[5][:, :case[1]], ops[6])
    got = out[:, :width].astype(np.float64)
    ratio = np.abs(got - ref) / bound
    print(f"[fp8] gemm {case}: worst |err| / bound {ratio.max():.3f}, max |ref| {np.abs(ref).max():.4g}")
    assert np.isfinite(got).all() and (out[:, width:] == 123.0).all()
    assert (ratio <= 1.0).all(), (case, int((ratio > 1).sum()), np.unravel_index(ratio.argmax(), ratio.shape))


def bitwise_cases(tsd_mod, repeats):
    """[(name, [digest per repeat])]: the GEMM at three shapes (one to ten K steps, partial tiles, GEGLU) and the widest quantiser."""
    out = []
    for case in (GEMM_CASES[2], GEMM_CASES[4], GEMM_CASES[5]):
        ops = gemm_case(*case)
        out.append((str(case), [hashlib.sha1(run_gemm(tsd_mod, ops)[0].tobytes()).hexdigest() for _ in range(repeats)]))
    x = quant_input(*QUANT_SHAPES[3])
    out.append(("quant", [hashlib.sha1(b"".join(a.tobytes() for a in tsd_mod.quant_rows_e4m3(x))).hexdigest() for _ in range(repeats)]))
    return out


def test_bits_do_not_depend_on_the_run_nor_on_the_jitter_build(gpu_ctx, tsd_mod):
    here = bitwise_cases(tsd_mod, 3)
    assert all(len(set(d)) == 1 for _, d in here), here
    if not os.path.exists(JITTER_LIB):
        pytest.skip(f"{JITTER_LIB} not built (`make -C stable-diffusion.mojo_amd/csrc jitter`; __graft_entry__.build() builds it)")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "jitter-child", str(JITTER_REPEATS)], env=dict(os.environ, TSD_LIB=JITTER_LIB),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert out.returncode == 0, f"the jitter child ended with status {out.returncode}:\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    there = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [t["name"] for t in there] == [n for n, _ in here]
    for (name, mine), theirs in zip(here, there):
        assert len(theirs["digests"]) == JITTER_REPEATS and all(dg == mine[0] for dg in theirs["digests"]), name


def test_linear_fp8_is_the_fake_quant_linear(gpu_ctx, tsd_mod):
    x, w, b = rng.normal(5, 1, 33 * 200).reshape(33, 200), rng.normal(5, 2, 50 * 200).reshape(50, 200) * 0.1, rng.normal(5, 3, 50)
    got, want = tsd_mod.linear_fp8(x, w, b), R.fake_quant_linear(x, w, b)
    assert rel_l2(got, want) < 2.0 ** -10 and 1e-2 < rel_l2(got, x @ w.T + b) < 6e-2   # fp16 store; and the operands really were 8-bit


# ---- the model option ---------------------------------------------------------------------------------------------------------------------
import freeu_ref as F   # the full-size restatement and the draws of the model-level tests (no table: the plain forward)


@pytest.fixture(scope="module", params=list(F.MODEL_KINDS))
def world(request, gpu_ctx, tsd_mod):
    """One kind (6, 16) with numpy-drawn parameters; B = 2 at 16 x 16; the fake-quant and the unquantised reference, computed once."""
    from controlnet_ref import draw_params
    from oracle import models
    kind = request.param
    P = draw_params(tsd_mod.param_specs(kind), F.MODEL_SEED)
    one = F.model_inputs(kind, 16, 16)
    two = [np.concatenate([a, np.ascontiguousarray(a[..., ::-1]) * 0.8]) for a in one[:2]] + [np.concatenate([one[2], one[2]])]
    plain_lin, cache = models._lin, {}

    def lin(P_, name, x, use_bias=True):   # the two feed-forward linears of every attention block: `unet.layerN.layer8` / `.layer9`
        if not name.endswith((".layer8", ".layer9")):
            return plain_lin(P_, name, x, use_bias)
        if name not in cache:
            q, s = R.quant_rows(P_[name + ".weight"].astype(np.float16))
            cache[name] = (R.E4M3[q] * s[:, None].astype(np.float64)).T
        q, s = R.quant_rows(np.asarray(x, np.float16))
        return ((R.E4M3[q] * s[:, None].astype(np.float64)) @ cache[name] + P_[name + ".bias"]).astype(np.float32)

    refs = {}
    for key, fn in (("plain", plain_lin), ("fp8", lin)):
        models._lin = fn
        try:
            refs[key] = np.stack([F.diffusion_freeu(P, two[0][b], two[1][b], two[2][b], None, steps=F.model_steps(kind), tn=True) for b in range(2)])
        finally:
            models._lin = plain_lin
    d = tsd_mod.Diffusion(params=P, variant=kind)
    yield kind, d, two, refs
    d.model.close()


def test_forward_with_the_option_matches_the_fake_quant_reference(world, tsd_mod):
    """Measured on an MI355X: 8.8e-3 (kind 6) and 9.6e-3 (kind 16) against the fake-quant reference - close to the model tolerance: the
    device quantises its own fp16 activations, the reference its float ones, and a last-bit difference flips e4m3 roundings - and 1.35e-2 /
    1.46e-2 against the unquantised reference (reported, the price of the data type; the fp16 path is at 1.25e-3 / 1.36e-3)."""
    kind, d, x, refs = world
    never = d.forward(*x)
    d.set_ff_fp8(True)
    try:
        assert d.ff_fp8
        on = d.forward(*x)
        alone = d.forward(*[a[1:2] for a in x])
        third = d.forward(*[np.concatenate([a[:1], a[:1], a[1:2]]) for a in x])
    finally:
        d.set_ff_fp8(False)
    off = d.forward(*x)
    print(f"[fp8] {kind}: option on against the fake-quant reference {rel_l2(on, refs['fp8']):.3e}, against the unquantised reference "
          f"{rel_l2(on, refs['plain']):.3e} (option off: {rel_l2(never, refs['plain']):.3e}); on against off {rel_l2(on, never):.3e}")
    assert np.isfinite(on).all() and rel_l2(on, refs["fp8"]) <= TOL_MODEL
    assert rel_l2(on, never) > 1e-3                      # the option acts ...
    assert np.array_equal(off, never) and not d.ff_fp8   # ... and off again gives the never-set bits
    assert np.array_equal(alone[0], on[1]) and np.array_equal(third[2], on[1])   # per-row scales: a sample's bits wherever it sits


def test_refused_kinds_and_values(gpu_ctx, tsd_mod):
    lib, dec = tsd_mod._lib.lib(), tsd_mod.Model("decoder", seed=1)
    try:
        assert lib.tsd_model_set_ff_fp8(dec.h, 1) == tsd_mod._lib.TSD_E_ARG and lib.tsd_model_ff_fp8(dec.h) == tsd_mod._lib.TSD_E_ARG
    finally:
        dec.close()
    with pytest.raises(tsd_mod.TsdError):
        tsd_mod.quant_rows_e4m3(np.zeros((2, 5128), np.float16))   # K > 5120


def test_cfg_session_with_the_option_equals_the_host_driven_loop_bitwise(gpu_ctx, tsd_mod):
    import test_gpu_controlnet as TC   # the host-driven loop and the session driver: the option is state of the model they drive
    case, inputs = TC.S_CASES[0], TC._s_inputs(2100)   # seeded DDPM
    d = tsd_mod.Diffusion(seed=TC.SEED, variant="diffusion_sd15")
    try:
        with TC.hoist(tsd_mod, gpu_ctx, 1):
            plain = TC.session_run(tsd_mod, d, None, case, True, inputs, None)
            d.set_ff_fp8(True)
            got = TC.session_run(tsd_mod, d, None, case, True, inputs, None)
            want = TC.host_loop(tsd_mod, gpu_ctx, d, None, case, True, inputs, lambda i: None)
    finally:
        d.model.close()
    assert all(np.isfinite(g).all() and TC._same(g, w) for g, w in zip(got, want)) and rel_l2(got[-1], plain[-1]) > 1e-4


if __name__ == "__main__":
    assert sys.argv[1] == "jitter-child"
    import tsd
    tsd.set_strict(True)
    for _name, _digests in bitwise_cases(tsd, int(sys.argv[2])):
        print(json.dumps({"name": _name, "digests": _digests}), flush=True)
