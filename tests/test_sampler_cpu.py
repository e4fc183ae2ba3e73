"""Host side of the DDIM / DPM-Solver++(2M) samplers (no GPU): the timestep lists and per-step scalars of `tsd_sampler_timesteps` /
`tsd_sampler_coeffs` (csrc/sampler.cpp) against
  - the oracle's DDPMSampler (the reference's timestep rule, and its DDPM step as DDIM with eta = 1),
  - an fp64 restatement of the published updates in the papers' own form (tests/sampler_ref.py: an update FUNCTION of x, eps, the
    previous data prediction and the noise; its linear coefficients are read off by probing it, nothing is expanded by hand),
  - a property of any consistent solver (a constant data prediction is reproduced at every step),
and the Python mirrors in tsd/sampler.py."""
import ctypes as C
import inspect

import numpy as np
import pytest

from oracle import sampler as osampler
from sampler_ref import N_TRAIN, Papers
from util import randn, rel_l2

KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}
SPACINGS = {"leading": 0, "trailing": 1}


@pytest.fixture(scope="module")
def lib(tsd_mod):
    return tsd_mod._lib.lib()


def c_timesteps(lib, spacing, n, start=0, n_train=N_TRAIN):
    buf = (C.c_int * n)()
    cnt = lib.tsd_sampler_timesteps(SPACINGS[spacing], n_train, n, start, buf, n)
    assert cnt == n - start, (cnt, lib.tsd_last_error())
    return [buf[k] for k in range(cnt)]


def c_coeffs(lib, kind, eta, spacing, n, i, have_history, start=0, n_train=N_TRAIN):
    out = (C.c_double * 8)()
    rc = lib.tsd_sampler_coeffs(KINDS[kind], float(eta), SPACINGS[spacing], n_train, n, start, i, int(have_history), out)
    assert rc == 0, lib.tsd_last_error()
    return np.array(out[:], dtype=np.float64)


# ---- 1. timesteps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 20, 50])
def test_leading_timesteps_are_the_reference_rule(lib, n):
    s = osampler.DDPMSampler(N_TRAIN)
    s.set_inference_timesteps(n)
    assert c_timesteps(lib, "leading", n) == [int(t) for t in s.timesteps]
    for strength in (1.0, 0.8, 0.6, 0.35):
        s = osampler.DDPMSampler(N_TRAIN)
        s.set_inference_timesteps(n)
        s.set_strength(strength)
        if s.start_step >= n:
            continue  # the slice is empty: no schedule
        assert c_timesteps(lib, "leading", n, s.start_step) == [int(t) for t in s.timesteps], (n, strength)


@pytest.mark.parametrize("n", [1, 3, 16, 20, 50, 1000])
def test_trailing_timesteps(lib, n):
    ts = c_timesteps(lib, "trailing", n)
    assert ts[0] == N_TRAIN - 1 and ts[-1] >= 0 and len(ts) == n
    assert all(a > b for a, b in zip(ts, ts[1:]))
    assert ts == [int(np.round(N_TRAIN - k * (N_TRAIN / n))) - 1 for k in range(n)]
    assert c_timesteps(lib, "trailing", n, n // 2) == ts[n // 2:]


def test_bad_arguments_are_refused(lib):
    out, buf = (C.c_double * 8)(), (C.c_int * 8)()
    assert lib.tsd_sampler_timesteps(2, 1000, 5, 0, buf, 8) == -1          # spacing
    assert lib.tsd_sampler_timesteps(0, 1000, 5, 5, buf, 8) == -1          # start_step >= n
    assert lib.tsd_sampler_timesteps(0, 10, 11, 0, buf, 8) == -1           # n > N
    assert lib.tsd_sampler_coeffs(3, 0.0, 0, 1000, 5, 0, 0, 0, out) == -1  # kind
    assert lib.tsd_sampler_coeffs(1, -0.5, 0, 1000, 5, 0, 0, 0, out) == -1  # eta < 0
    assert lib.tsd_sampler_coeffs(1, 0.0, 0, 1000, 5, 0, 5, 0, out) == -1  # step out of range
    assert lib.tsd_sampler_coeffs(1, 0.0, 0, 1000, 5, 0, 0, 0, None) == -1
    assert lib.tsd_sampler_timesteps(1, 1000, 20, 0, None, 0) == 20        # NULL only asks for the count


# ---- 2. the published updates, restated in fp64 (sampler_ref.Papers) ------------------------------------------------------------
def _cases():
    for spacing in ("leading", "trailing"):
        for n in (3, 20, 50):
            for hist in (0, 1):
                yield ("ddpm", 0.0, spacing, n, hist)
                yield ("dpmpp_2m", 0.0, spacing, n, hist)
                for eta in (0.0, 0.5, 1.0):
                    yield ("ddim", eta, spacing, n, hist)


@pytest.mark.parametrize("kind,eta,spacing,n,hist", list(_cases()))
def test_coefficients_match_the_papers_in_fp64(lib, kind, eta, spacing, n, hist):
    """Both sides are a dozen double operations on the same fp32 table: |delta| <= 1e-12 * max(1, |c|)."""
    ts = c_timesteps(lib, spacing, n)
    P = Papers(ts)
    update = {"ddpm": P.ddpm, "ddim": P.ddim(eta), "dpmpp_2m": P.dpmpp_2m}[kind]
    worst = 0.0
    for i in range(n):
        got = c_coeffs(lib, kind, eta, spacing, n, i, hist)
        assert got[0] == ts[i] and got[1] == (ts[i + 1] if i + 1 < n else -1)
        want = P.linear_form(update, i, bool(hist))
        err = np.abs(got[2:] - want) / np.maximum(1.0, np.abs(want))
        worst = max(worst, err.max())
        assert err.max() <= 1e-12, (kind, eta, spacing, n, i, hist, got[2:], want)
        if kind != "dpmpp_2m" or not hist or i == 0 or i == n - 1:
            assert got[6] == 0.0                       # no history term outside the second-order steps
        else:
            assert got[6] != 0.0
        if kind == "dpmpp_2m" or (kind == "ddim" and eta == 0.0):
            assert got[7] == 0.0                       # deterministic
    print(f"[sampler] {kind} eta={eta} {spacing} n={n} hist={hist}: worst |delta|/max(1,|c|) = {worst:.2e}")


def test_start_step_drops_leading_entries_for_every_sampler(lib):
    """img2img: the scalars of step i of a schedule that starts at `start` are those of step start + i of the full one, except that
    the multistep solver has no history on its first step."""
    n, start = 20, 8
    for kind, eta in (("ddpm", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)):
        for spacing in ("leading", "trailing"):
            for i in range(n - start):
                a = c_coeffs(lib, kind, eta, spacing, n, i, 1, start=start)
                b = c_coeffs(lib, kind, eta, spacing, n, start + i, 0 if i == 0 else 1)
                assert np.array_equal(a, b), (kind, spacing, i)


# ---- 3. tie to the reference: DDIM(eta = 1, LEADING) is the reference's DDPM step -------------------------------------------------
@pytest.mark.parametrize("n", [3, 20, 50])
def test_ddim_eta1_is_the_reference_ddpm_step(lib, n):
    """The oracle's `DDPMSampler.coefficients` (fp32 scalar arithmetic, like the reference) folded to the linear form
    c_x = c_xt + c_x0 / sqrt(a_t), c_e = -c_x0 sqrt(1 - a_t) / sqrt(a_t), c_n = sigma.  The two forms agree to 3e-15 in fp64; the
    oracle's fp32 scalars put 1.2e-7 (n = 3), 2.6e-7 (n = 20), 1.4e-6 (n = 50) between them.  Bar 1e-5: the figure
    test_cfg_batch_equals_two_passes uses for this sampler's fp32 algebra."""
    s = osampler.DDPMSampler(N_TRAIN)
    s.set_inference_timesteps(n)
    x, eps, z = (randn(900 + k, 4, 8, 8).astype(np.float32) for k in range(3))
    worst_c = worst_u = 0.0
    for i, t in enumerate(int(t) for t in s.timesteps):
        sa, sb, c_x0, c_xt, sigma = (np.float64(v) for v in s.coefficients(t))
        want = np.array([c_xt + c_x0 / sa, -c_x0 * sb / sa, sigma])
        got = c_coeffs(lib, "ddim", 1.0, "leading", n, i, 0)
        assert got[0] == t and got[6] == 0.0
        have = got[[4, 5, 7]]
        worst_c = max(worst_c, (np.abs(have - want) / np.maximum(1.0, np.abs(want))).max())
        ref = s.step(t, x, eps, z)
        upd = have[0] * x.astype(np.float64) + have[1] * eps.astype(np.float64) + have[2] * z.astype(np.float64)
        worst_u = max(worst_u, rel_l2(upd, ref))
    print(f"[sampler] DDIM(1) vs the oracle's DDPM step, n={n}: coefficients {worst_c:.2e}, one update rel_l2 {worst_u:.2e}")
    assert worst_c <= 1e-5 and worst_u <= 1e-5


# ---- 4. a property of the solvers, independent of any restatement ----------------------------------------------------------------
@pytest.mark.parametrize("kind,hist", [("ddim", 0), ("dpmpp_2m", 0), ("dpmpp_2m", 1)])
@pytest.mark.parametrize("spacing", ["leading", "trailing"])
@pytest.mark.parametrize("n", [3, 20])
def test_constant_data_prediction_is_reproduced(lib, kind, hist, spacing, n):
    """If the model's eps encodes the same x0 = c at every step (eps = (x - alpha_t c) / sigma_t), every step of a consistent solver
    lands on alpha_p c + (sigma_p / sigma_t) (x - alpha_t c), and the last one on c itself (sigma_p = 0: no remainder term)."""
    ab = osampler.DDPMSampler(N_TRAIN).alphas_cumprod.astype(np.float64)
    c = randn(910, 4, 8, 8).astype(np.float64)
    x = randn(911, 4, 8, 8).astype(np.float64)
    h = None
    for i in range(n):
        t, tp, al, sg, c_x, c_e, c_h, c_n = c_coeffs(lib, kind, 0.0, spacing, n, i, hist and h is not None)
        assert c_n == 0.0
        eps = (x - al * c) / sg
        a_p = ab[int(tp)] if tp >= 0 else 1.0
        want = np.sqrt(a_p) * c + np.sqrt(1 - a_p) / sg * (x - al * c)
        new = c_x * x + c_e * eps + (c_h * h if h is not None else 0.0)
        scale = np.abs(x).max() / al + np.abs(c).max()
        assert np.abs(new - want).max() <= 1e-12 * scale, (kind, spacing, n, i)
        h = (x - sg * eps) / al                       # the data prediction the kernel keeps: c up to rounding
        x = new
    assert np.abs(x - c).max() <= 1e-12 * (np.abs(c).max() + 1.0)


# ---- 5. mirrors and defaults ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["leading", "trailing"])
def test_python_mirrors_return_what_the_library_returns(lib, tsd_mod, spacing):
    n, strength = 20, 0.6
    for kind, eta, make in (("ddim", 0.0, lambda: tsd_mod.DDIMSampler(N_TRAIN, 0.0, spacing)),
                            ("ddim", 0.5, lambda: tsd_mod.DDIMSampler(N_TRAIN, 0.5, spacing)),
                            ("dpmpp_2m", 0.0, lambda: tsd_mod.DPMSolverMultistepSampler(N_TRAIN, spacing))):
        for start_from_strength in (False, True):
            m = make()
            m.set_inference_timesteps(n)
            if start_from_strength:
                m.set_strength(strength)
            start = m.start_step
            assert [int(t) for t in m.timesteps] == c_timesteps(lib, spacing, n, start)
            for i in range(len(m.timesteps)):
                for hist in (0, 1):
                    got = np.array(m.coefficients(i, bool(hist)), dtype=np.float64)
                    want = c_coeffs(lib, kind, eta, spacing, n, i, hist, start=start)
                    assert np.array_equal(got[:2], want[:2])
                    assert (np.abs(got[2:] - want[2:]) <= 1e-12 * np.maximum(1.0, np.abs(want[2:]))).all(), (kind, i, hist)


def test_generate_defaults_are_the_reference_loop(tsd_mod):
    p = inspect.signature(tsd_mod.generate).parameters
    assert (p["sampler"].default, p["eta"].default, p["spacing"].default) == ("ddpm", 0.0, "leading")
    p = inspect.signature(tsd_mod.Session.set_sampler).parameters
    assert (p["kind"].default, p["eta"].default, p["spacing"].default) == ("ddpm", 0.0, "leading")
    from tsd import _lib
    assert _lib.SAMPLER_KINDS == KINDS and _lib.TIMESTEP_SPACINGS == SPACINGS
