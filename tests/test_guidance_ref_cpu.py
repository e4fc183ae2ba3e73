"""Guidance rescale without a GPU: the fp64 reference (tests/guidance_ref.py) against a float64 restatement of diffusers' `rescale_noise_cfg`,
its exact cases, the argument checks of the C ABI and the host layers, and the Mojo shim's symbols."""
import os

import numpy as np
import pytest

import guidance_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
SYMBOLS = ["tsd_cfg_rescale_f32", "tsd_ddpm_step_f32", "tsd_session_set_guidance_rescale", "tsd_session_guidance_rescale",
           "tsd_session_slot_set_guidance_rescale", "tsd_session_slot_guidance_rescale"]


def _families(tsd_mod, n, B=3):
    z = [tsd_mod.rng.normal(SEED, 2000 + k, B * n).reshape(B, n).astype(np.float32) for k in range(2)]
    yield "independent", z[0], z[1]
    yield "near", z[0], (z[0] + np.float32(0.1) * z[1]).astype(np.float32)
    yield "offset", (np.float32(0.1) + np.float32(0.01) * z[0]).astype(np.float32), (np.float32(0.1) + np.float32(0.01) * z[1]).astype(np.float32)


@pytest.mark.parametrize("n", [4, 260, 2304, 16384])
def test_reference_agrees_with_the_diffusers_formula_in_float64(tsd_mod, n):
    """diffusers' rescale_noise_cfg, restated in torch float64: the unbiased std over all non-batch dimensions of the conditional and of the
    combined prediction, factor = phi * std_c / std_e + (1 - phi).  The std is written out as the two-pass formula on torch's pairwise sums
    (torch.std's streaming update drifts by tens of ulps at n = 16384, which would be the comparator's error, not the reference's): a
    two-pass variance is well conditioned, so each carries (log2 n + 4) 2^-53, and the ratio's square root as much.  The reference takes the
    variances in ONE pass: numpy's pairwise float64 sums carry at most (log2 n + 2) 2^-53 each, which the subtraction magnifies by kappa; two
    variances and a square root leave 2 (log2 n + 2) 2^-53 kappa on g.  BOUND = (2 (log2 n + 2) kappa + 2 (log2 n + 4)) 2^-53, relative."""
    import torch

    def std(t):
        d = t - t.mean(dim=1, keepdim=True)
        return torch.sqrt((d * d).sum(dim=1) / (t.shape[1] - 1))

    for name, c, u in _families(tsd_mod, n):
        for s, phi in ((7.5, 0.7), (12.0, 1.0), (3.0, 0.3)):
            e = gr.combine_f32(c, u, s)
            tc, te = torch.from_numpy(c.astype(np.float64)), torch.from_numpy(e.astype(np.float64))
            std_c, std_e = std(tc), std(te)
            want = (float(np.float32(phi)) * (std_c / std_e) + (1.0 - float(np.float32(phi)))).numpy()
            _, _, g32, g64, kappa = gr.rescale(c, u, s, phi)
            bound = (2 * (np.log2(n) + 2) * kappa + 2 * (np.log2(n) + 4)) * 2.0 ** -53
            rel = np.abs(g64 - want) / np.abs(want)
            assert (rel <= bound).all(), (name, n, s, phi, rel.tolist(), bound.tolist())
            assert np.array_equal(g32, g64.astype(np.float32))


def test_offset_family_conditioning_is_what_the_gpu_test_relies_on(tsd_mod):
    """c = 0.1 + 0.01 z has kappa about 102: n 2^-53 kappa = 1.9e-10 < 2^-30 at n = 16384, so no float64 summation order moves g visibly - and
    a float32 accumulation (n 2^-24 kappa, far above one float32 ulp) would."""
    n = 16384
    _, c, u = list(_families(tsd_mod, n))[2]
    _, _, _, _, kappa = gr.rescale(c, u, 7.5, 0.7)
    assert (kappa > 90).all() and (kappa < 115).all(), kappa
    assert (n * 2.0 ** -53 * kappa < 2.0 ** -30).all()
    assert (n * 2.0 ** -24 * kappa > 100 * 2.0 ** -24).all()


def test_exact_cases(tsd_mod):
    n = 2304
    _, c, u = next(_families(tsd_mod, n))
    # phi = 0: g = 1 and the sample is its input, whatever the scale
    co, uo, g32, g64, _ = gr.rescale(c, u, 7.5, 0.0)
    assert (g64 == 1.0).all() and (g32 == 1.0).all() and np.array_equal(co.view(np.uint32), c.view(np.uint32)) and np.array_equal(uo.view(np.uint32), u.view(np.uint32))
    # s = 1 on values for which (c - u) + u is exact (multiples of 2^-8 below 8): e is c, the variances are equal and g = 1 for every phi
    cq, uq = (np.round(c * 256) / 256).astype(np.float32), (np.round(u * 256) / 256).astype(np.float32)
    assert np.array_equal(gr.combine_f32(cq, uq, 1.0), cq)
    for phi in (0.3, 0.7, 1.0):
        assert (gr.rescale(cq, uq, 1.0, phi)[3] == 1.0).all(), phi
    # degenerate: constant tensors (var_e <= 0 or the ratio of two equal variances) and a NaN give g = 1
    k = np.full((2, n), 0.37, dtype=np.float32)
    assert (gr.rescale(k, k, 7.5, 0.7)[3] == 1.0).all()
    bad = c.copy()
    bad[1, 5] = np.nan
    g = gr.rescale(bad, u, 7.5, 0.7)[3]
    assert g[1] == 1.0 and g[0] != 1.0 and g[2] != 1.0
    # mixed per-sample phi: row b follows phi[b]
    phis = np.array([0.0, 0.7, 1.0], dtype=np.float32)
    g = gr.rescale(c, u, 7.5, phis)[3]
    assert g[0] == 1.0 and g[1] == gr.rescale_factor(c[1], u[1], 7.5, 0.7)[0] and g[2] == gr.rescale_factor(c[2], u[2], 7.5, 1.0)[0]
    assert 0.0 < g[2] < g[1] < 1.0   # guidance at 7.5 inflates the deviation: the rescale shrinks


def test_symbols_are_declared_exported_and_refuse_bad_arguments(tsd_mod):
    from tsd._lib import TSD_E_ARG, TSD_E_SHAPE, ptr
    lib = tsd_mod._lib.lib()
    declared = tsd_mod._lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    x = np.zeros(3 * 16, dtype=np.float32)
    s, phi, g = np.full(3, 7.5, dtype=np.float32), np.full(3, 0.7, dtype=np.float32), np.zeros(3, dtype=np.float32)

    def op(eps=x, u=x, B=3, chw=16, s=s, phi=phi, out=x):
        return lib.tsd_cfg_rescale_f32(None, ptr(eps), ptr(u), B, chw, ptr(s), ptr(phi), ptr(out), ptr(out), ptr(g))

    assert op(B=0) == TSD_E_SHAPE and op(B=17) == TSD_E_SHAPE and op(chw=0) == TSD_E_SHAPE and op(chw=-4) == TSD_E_SHAPE
    for bad in (-0.1, 1.5, np.nan, np.inf):
        assert op(phi=np.array([0.7, bad, 0.0], dtype=np.float32)) == TSD_E_ARG, bad
        assert b"phi[1]" in lib.tsd_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        assert op(s=np.array([7.5, 7.5, bad], dtype=np.float32)) == TSD_E_ARG, bad
    assert op(eps=None) == TSD_E_ARG and op(u=None) == TSD_E_ARG and op(phi=None) == TSD_E_ARG and op(s=None) == TSD_E_ARG and op(out=None) == TSD_E_ARG
    assert op() == TSD_E_ARG and b"ctx" in lib.tsd_last_error()   # valid arguments reach the context check: no GPU, no CPU fallback
    one = np.zeros(1, dtype=np.float32)
    assert lib.tsd_session_set_guidance_rescale(None, 0.7) == TSD_E_ARG and b"NULL" in lib.tsd_last_error()
    assert lib.tsd_session_guidance_rescale(None, ptr(one)) == TSD_E_ARG
    assert lib.tsd_session_slot_set_guidance_rescale(None, 0, 0.7) == TSD_E_ARG
    assert lib.tsd_session_slot_guidance_rescale(None, 0, ptr(one)) == TSD_E_ARG
    assert lib.tsd_ddpm_step_f32(None, ptr(x), ptr(x), None, 7.5, None, 0, 0, 1000, 4, 0, 0, ptr(x)) == TSD_E_SHAPE
    assert lib.tsd_ddpm_step_f32(None, ptr(x), ptr(x), None, 7.5, None, 48, 0, 1000, 4, 0, 4, ptr(x)) == TSD_E_ARG   # step 4 of 4
    for name in ("set_guidance_rescale", "slot_set_guidance_rescale", "slot_guidance_rescale"):
        assert callable(getattr(tsd_mod.Session, name)), name
    assert isinstance(tsd_mod.Session.guidance_rescale, property)


def test_host_layers_refuse_bad_values_before_the_library(tsd_mod):
    c = np.zeros((2, 4, 2, 2), dtype=np.float32)
    for bad in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match="between 0 and 1"):
            tsd_mod.cfg_rescale(c, c, 7.5, bad)
        with pytest.raises(ValueError, match="between 0 and 1"):
            tsd_mod.cfg_rescale(c, c, 7.5, [0.5, bad])
    with pytest.raises(ValueError, match="finite"):
        tsd_mod.cfg_rescale(c, c, [7.5, float("inf")], 0.7)
    with pytest.raises(ValueError, match="same"):
        tsd_mod.cfg_rescale(c, c[:1], 7.5, 0.7)

    class NoLibrary:   # the session methods check the value before they touch the handle
        h, cfg = None, True

    for method, args in ((tsd_mod.Session.set_guidance_rescale, ()), (tsd_mod.Session.slot_set_guidance_rescale, (0,))):
        for bad in (-0.5, 2.0, float("nan")):
            with pytest.raises(ValueError, match="between 0 and 1"):
                method(NoLibrary(), *args, bad)
        nocfg = NoLibrary()
        nocfg.cfg = False
        with pytest.raises(ValueError, match="cfg=True"):
            method(nocfg, *args, 0.7)


def test_generate_and_request_validation(tsd_mod):
    from tsd.serve import Request, SlotScheduler
    ctx = np.zeros((1, 77, 768), dtype=np.float32)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            tsd_mod.generate(None, None, ctx, uncond_context=ctx, guidance_rescale=bad)
    with pytest.raises(ValueError, match="cfg=True"):
        tsd_mod.generate(None, None, ctx, cfg=False, guidance_rescale=0.7)
    assert Request(1, ctx[0]).guidance_rescale == 0.0 and Request(1, ctx[0], guidance_rescale=0.7).guidance_rescale == 0.7
    # the keyword rides beside the nine positional fields: tuples in their order still make a Request, and _replace keeps it
    assert Request._fields == ("id", "context", "uncond", "seed", "cfg_scale", "latents", "strength", "mask", "mask_mode")
    r = Request(*tuple(Request(2, ctx[0], ctx[0], 9, 3.0)), guidance_rescale=0.3)
    assert (r.seed, r.cfg_scale, r.guidance_rescale) == (9, 3.0, 0.3) and len(r) == 9
    assert r._replace(seed=4).guidance_rescale == 0.3 and r._replace(guidance_rescale=0.5).guidance_rescale == 0.5 and r._replace(seed=4).seed == 4
    assert Request._make(tuple(r)).guidance_rescale == 0.0
    for bad in (-0.1, 1.2, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            Request(1, ctx[0], guidance_rescale=bad)

    class Fake:
        """The slot methods the scheduler calls, recording them."""
        B, L, num_steps, cfg = 2, 2, 2, True

        def __init__(self):
            self.events, self.left = [], {}

        def slot_start(self, b, context, uncond_context=None, **kw):
            self.left[b] = self.num_steps
            self.events.append(("start", b, kw["cfg_scale"]))

        def slot_set_guidance_rescale(self, b, phi):
            assert b in self.left
            self.events.append(("rescale", b, phi))

        def advance(self):
            done = []
            for b in sorted(self.left):
                self.left[b] -= 1
                if not self.left[b]:
                    done.append(b)
            for b in done:
                del self.left[b]
            self.events.append(("advance",))
            return done

        def slot_latents(self, b):
            return np.zeros((4, 2, 2), dtype=np.float32)

    f = Fake()
    reqs = [Request("a", ctx[0], ctx[0], 1, 7.5), Request("b", ctx[0], ctx[0], 2, 9.0, guidance_rescale=0.7), Request("c", ctx[0], ctx[0], 3, 5.0, guidance_rescale=0.3)]
    assert [rid for rid, _ in SlotScheduler(f, reqs)] == ["a", "b", "c"]
    # a request at 0 makes no call; the others set their own value right after their slot_start, before the next advance
    assert f.events == [("start", 0, 7.5), ("start", 1, 9.0), ("rescale", 1, 0.7), ("advance",), ("advance",), ("start", 0, 5.0), ("rescale", 0, 0.3),
                        ("advance",), ("advance",)]
    # a request that cannot run raises before its slot is touched
    f = Fake()
    r = Request("x", ctx[0], ctx[0], 1, 7.5)
    r.guidance_rescale = 1.2   # set behind the constructor's back: the scheduler checks again
    with pytest.raises(ValueError, match="guidance_rescale"):
        list(SlotScheduler(f, [r]))
    assert f.events == []
    f = Fake()
    f.cfg = False
    with pytest.raises(ValueError, match="cfg=True"):
        list(SlotScheduler(f, [Request("x", ctx[0], None, 1, 7.5, guidance_rescale=0.7)]))
    assert f.events == []


def test_mojo_shim_and_header_name_every_new_symbol():
    shim = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "mojo_shim", "tsd_ffi.mojo")).read()
    header = open(os.path.join(ROOT, "include", "tsd.h")).read()
    for name in SYMBOLS:
        assert f'"{name}"' in shim and f"int {name}(" in header, name
    dshim = open(os.path.join(ROOT, "stable-diffusion.mojo_amd", "mojo_shim", "diffusion_shim.mojo")).read()
    for call in ("self.tsd.cfg_rescale(", "self.tsd.session_set_guidance_rescale(", "self.tsd.session_slot_set_guidance_rescale("):
        assert call in dshim, call
