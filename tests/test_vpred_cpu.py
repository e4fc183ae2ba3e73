"""Host side of v-prediction and the zero-terminal-SNR table (no GPU): `tsd_sampler_alphas_cumprod` and `tsd_sampler_coeffs_ex`
(csrc/sampler.cpp) against
  - the fp64 restatement of Lin et al. 2023 algorithm 1 and of the three updates with x0 = alpha x - sigma v, eps = sigma x + alpha v
    substituted into the papers' equations (tests/vpred_ref.py),
  - the library's own epsilon rows (c_x^v = c_x^e + c_e^e sigma, c_v = c_e^e alpha wherever alpha_t > 0),
  - the terminal step (abar_t = 0), where every output must be finite,
  - a property of any consistent solver (a constant data prediction is reproduced, from pure noise),
and the Python side: mirrors, `read_scheduler_config`, defaults.

The coefficient agreements are held to forward error bounds that nobody chose: both sides of a comparison are evaluated on
vpred_ref.Err numbers (one 2^-53 rounding per double operation, propagated through the expression as written), and the difference must
stay within the sum of the two bounds.  The library's side of that is `_rows`, the rows of sampler.cpp as include/tsd.h and the issue
state them, restated here on Err numbers for the BOUND only; the values compared are the library's."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import vpred_ref as R
from test_sampler_cpu import _cases
from util import randn

KINDS = {"ddpm": 0, "ddim": 1, "dpmpp_2m": 2}
SPACINGS = {"leading": 0, "trailing": 1}
EPS, V = 0, 1
N_TRAIN = R.N_TRAIN
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib(tsd_mod):
    return tsd_mod._lib.lib()


def c_table(lib, n_train, ztsnr):
    buf = (C.c_float * n_train)()
    assert lib.tsd_sampler_alphas_cumprod(n_train, int(ztsnr), buf, n_train) == n_train, lib.tsd_last_error()
    return np.array(buf[:], dtype=np.float32)


def c_timesteps(lib, spacing, n, start=0, n_train=N_TRAIN):
    buf = (C.c_int * n)()
    cnt = lib.tsd_sampler_timesteps(SPACINGS[spacing], n_train, n, start, buf, n)
    assert cnt == n - start
    return [buf[k] for k in range(cnt)]


def c_ex(lib, kind, eta, spacing, n, i, hist, pred, ztsnr, start=0, n_train=N_TRAIN, raw=False):
    out = (C.c_double * 8)()
    rc = lib.tsd_sampler_coeffs_ex(KINDS[kind], float(eta), SPACINGS[spacing], n_train, n, start, i, int(hist), pred, int(ztsnr), out)
    if raw:
        return rc
    assert rc == 0, lib.tsd_last_error()
    return np.array(out[:], dtype=np.float64)


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_train", [1000, 10])
def test_zero_terminal_snr_table(lib, n_train):
    plain, z = c_table(lib, n_train, 0), c_table(lib, n_train, 1)
    assert plain.tobytes() == R.plain_table(n_train).tobytes()              # flag 0: bitwise the table every session uses today
    assert z[-1] == 0.0 and np.signbit(z[-1]) == 0                          # exactly zero
    assert abs(np.float64(z[0]) - np.float64(plain[0])) <= np.spacing(plain[0])
    assert (np.diff(z.astype(np.float64)) < 0).all()                        # strictly decreasing
    want = R.zero_terminal_snr_table64(n_train).astype(np.float32)
    ulps = np.abs(z.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(want, np.float32(1e-45))).astype(np.float64)
    print(f"[vpred] table N={n_train}: worst distance from the fp64 restatement rounded to float = {ulps.max():.2f} ulp")
    assert ulps.max() <= 1.0


def test_table_entry_refuses_bad_arguments(lib):
    buf = (C.c_float * 4)()
    assert lib.tsd_sampler_alphas_cumprod(0, 0, buf, 4) == -1
    assert lib.tsd_sampler_alphas_cumprod(10, 2, buf, 4) == -1 and lib.tsd_sampler_alphas_cumprod(10, -1, buf, 4) == -1
    assert lib.tsd_sampler_alphas_cumprod(1, 1, buf, 4) == -1               # s_0 - s_{N-1} = 0: no rescale of a one-entry table
    assert lib.tsd_sampler_alphas_cumprod(10, 1, None, 0) == 10             # NULL only asks for the count
    assert lib.tsd_sampler_alphas_cumprod(10, 1, buf, 4) == 10 and buf[3] > 0.0   # cap < N: the first cap entries


# ---- 2. (epsilon, plain table) is tsd_sampler_coeffs ----------------------------------------------------------------------------------
def test_ex_with_the_defaults_is_tsd_sampler_coeffs_bitwise(lib):
    checked = 0
    for kind, eta, spacing, n, hist in _cases():
        for i in range(n):
            a, b = (C.c_double * 8)(), (C.c_double * 8)()
            assert lib.tsd_sampler_coeffs(KINDS[kind], eta, SPACINGS[spacing], N_TRAIN, n, 0, i, hist, a) == 0
            assert lib.tsd_sampler_coeffs_ex(KINDS[kind], eta, SPACINGS[spacing], N_TRAIN, n, 0, i, hist, EPS, 0, b) == 0
            assert bytes(a) == bytes(b), (kind, eta, spacing, n, i, hist)
            checked += 1
    assert checked > 1000


# ---- 3. the v rows ------------------------------------------------------------------------------------------------------------------
def _rows(kind, eta, a_t, a_p, a_l, last, pred):
    """The rows of csrc/sampler.cpp on Err numbers -> [c_x, c_e or c_v, c_h, c_n] with their forward error bounds.  a_l: abar of the step
    before (None: first order).  Epsilon: include/tsd.h "samplers" (x0 = (x - sigma e) / alpha); v: the rows of the v-prediction
    section, none of which divides by alpha_t."""
    E = R.Err
    one = E(1.0)
    al_t, sg_t, al_p, sg_p = R.sqrt(a_t), R.sqrt(one - a_t), R.sqrt(a_p), R.sqrt(one - a_p)
    zero = E(0.0)
    if kind == "ddpm":
        cur_a = a_t / a_p
        cur_b = one - cur_a
        c_x0, c_xt = al_p * cur_b / (one - a_t), R.sqrt(cur_a) * (one - a_p) / (one - a_t)
        c_n = zero if last else R.sqrt(((one - a_p) / (one - a_t) * cur_b).maxc(1e-20))
        if pred == V:
            return [c_xt + c_x0 * al_t, -(c_x0 * sg_t), zero, c_n]
        return [c_xt + c_x0 / al_t, -(c_x0 * sg_t / al_t), zero, c_n]
    if kind == "ddim":
        var = E(eta) * E(eta) * (one - a_p) / (one - a_t) * (one - a_t / a_p) if a_t.v > 0 else E(eta) * E(eta) * (one - a_p)
        d = R.sqrt((one - a_p - var).maxc(0.0))
        if pred == V:
            return [al_p * al_t + d * sg_t, d * al_t - al_p * sg_t, zero, R.sqrt(var)]
        c_x = R.sqrt(a_p / a_t)
        return [c_x, d - c_x * sg_t, zero, R.sqrt(var)]
    if last:
        return [al_t, -sg_t, zero, zero] if pred == V else [one / al_t, -(sg_t / al_t), zero, zero]
    w0, w1 = one, zero
    if a_t.v > 0:
        lam_t, lam_p = 0.5 * R.log(a_t / (one - a_t)), 0.5 * R.log(a_p / (one - a_p))
        h = lam_p - lam_t
        g = -(al_p * R.expm1(-h))
        if a_l is not None and a_l.v > 0:
            r = (lam_t - 0.5 * R.log(a_l / (one - a_l))) / h
            w1 = one / (2.0 * r)
            w0 = one + w1
    else:
        g = al_p
    if pred == V:
        return [sg_p / sg_t + g * w0 * al_t, -(g * w0 * sg_t), -(g * w1), zero]
    return [sg_p / sg_t + g * w0 / al_t, -(g * w0 * sg_t / al_t), -(g * w1), zero]


def _abar(tab, ts, i):
    return R.Err(float(tab[ts[i]])) if 0 <= i < len(ts) else R.Err(1.0)


TABLES = [(0, "leading"), (0, "trailing"), (1, "leading"), (1, "trailing")]


@pytest.mark.parametrize("ztsnr,spacing", TABLES)
def test_v_rows_agree_with_the_epsilon_rows_and_with_the_restatement(lib, ztsnr, spacing):
    """Wherever alpha_t > 0 the two forms are the same update: c_x^v = c_x^e + c_e^e sigma_t and c_v = c_e^e alpha_t (the library's
    epsilon rows, combined in double).  Everywhere - the terminal step included - the v rows are what probing vpred_ref.VPapers gives.
    Every difference is held to the sum of the two sides' running error bounds (module docstring), with both bounds printed."""
    tab = c_table(lib, N_TRAIN, ztsnr)
    worst = {"eps": 0.0, "ref": 0.0}
    largest_bound = 0.0
    n_eps = n_ref = 0
    for kind, eta, sp, n, hist in _cases():
        if sp != spacing:
            continue
        ts = c_timesteps(lib, spacing, n)
        eps_allowed = all(tab[t] > 0 for t in ts)
        P = R.VPapers(ts, tab, track=True)
        update = P.update(kind, eta)
        for i in range(n):
            got = c_ex(lib, kind, eta, spacing, n, i, hist, V, ztsnr)
            assert got[0] == ts[i] and got[1] == (ts[i + 1] if i + 1 < n else -1)
            assert np.isfinite(got).all()
            a_t, a_p = _abar(tab, ts, i), _abar(tab, ts, i + 1)
            a_l = _abar(tab, ts, i - 1) if (hist and i > 0 and kind == "dpmpp_2m") else None
            mine = _rows(kind, eta, a_t, a_p, a_l, i + 1 >= n, V)
            assert got[2] == np.sqrt(np.float64(tab[ts[i]])) and got[3] == np.sqrt(1.0 - np.float64(tab[ts[i]]))
            # (b) the restatement
            want = P.linear_form(update, i, bool(hist))
            for k in range(4):
                w = R.Err.of(want[2 + k])
                bound = w.e + mine[k].e
                diff = abs(got[4 + k] - w.v)
                largest_bound = max(largest_bound, bound)
                if bound > 0:
                    worst["ref"] = max(worst["ref"], diff / bound)
                assert diff <= bound, (kind, eta, spacing, n, i, hist, k, got[4 + k], w.v, bound)
                n_ref += 1
            # (a) the library's epsilon rows
            if eps_allowed:
                ge = c_ex(lib, kind, eta, spacing, n, i, hist, EPS, ztsnr)
                assert np.array_equal(ge[:4], got[:4]) and ge[6] == got[6] and ge[7] == got[7]   # c_h and c_n do not depend on the form
                er = _rows(kind, eta, a_t, a_p, a_l, i + 1 >= n, EPS)
                sg, al = R.sqrt(R.Err(1.0) - a_t), R.sqrt(a_t)
                for k, comb_bound, comb in ((0, er[0] + er[1] * sg, ge[4] + ge[5] * got[3]), (1, er[1] * al, ge[5] * got[2])):
                    bound = comb_bound.e + mine[k].e
                    diff = abs(got[4 + k] - comb)
                    worst["eps"] = max(worst["eps"], diff / bound)
                    assert diff <= bound, (kind, eta, spacing, n, i, hist, k, got[4 + k], comb, bound)
                    n_eps += 1
    print(f"[vpred] ztsnr={ztsnr} {spacing}: worst |delta| / bound  vs epsilon rows {worst['eps']:.3f} ({n_eps} scalars), "
          f"vs restatement {worst['ref']:.3f} ({n_ref} scalars); largest bound {largest_bound:.2e}")
    assert n_ref > 0 and (n_eps > 0) == (not (ztsnr and spacing == "trailing"))


# ---- 4. the terminal step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 20])
def test_terminal_step_is_finite_and_first_order(lib, n):
    rows = {}
    for kind, eta in (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)):
        for hist in (0, 1):
            c = c_ex(lib, kind, eta, "trailing", n, 0, hist, V, 1)
            assert np.isfinite(c).all(), (kind, eta, c)
            assert c[0] == N_TRAIN - 1 and c[2] == 0.0 and c[3] == 1.0       # alpha_t = 0, sigma_t = 1: x0 = -v
            rows[(kind, eta, hist)] = c
    for hist in (0, 1):
        assert np.array_equal(rows[("dpmpp_2m", 0.0, hist)], rows[("ddim", 0.0, 0)])   # h = +inf, g = alpha_p: the DDIM(0) step
    tab = c_table(lib, N_TRAIN, 1)
    a_p = np.float64(tab[int(rows[("ddim", 0.0, 0)][1])])
    d = rows[("ddim", 0.0, 0)]
    assert abs(d[4] - np.sqrt(1 - a_p)) <= 4 * R.U and abs(d[5] + np.sqrt(a_p)) <= 4 * R.U and d[7] == 0.0   # x' = alpha_p (-v) + sigma_p x
    e = rows[("ddim", 0.5, 0)]
    assert abs(e[7] - 0.5 * np.sqrt(1 - a_p)) <= 4 * R.U                     # var = eta^2 (1 - a_p) at abar_t = 0
    p = rows[("ddpm", 0.0, 0)]
    assert p[4] == 0.0 and abs(p[5] + np.sqrt(a_p)) <= 4 * R.U and abs(p[7] - np.sqrt(1 - a_p)) <= 4 * R.U
    # the step after the terminal one: r = +inf, no history term whatever the caller holds
    first, second = c_ex(lib, "dpmpp_2m", 0.0, "trailing", n, 1, 0, V, 1), c_ex(lib, "dpmpp_2m", 0.0, "trailing", n, 1, 1, V, 1)
    assert second[6] == 0.0 and np.array_equal(first, second)
    if n > 3:
        assert c_ex(lib, "dpmpp_2m", 0.0, "trailing", n, 2, 1, V, 1)[6] != 0.0   # ... and second order from there on


# ---- 5. a property of the solvers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hist", [("ddim", 0), ("dpmpp_2m", 0), ("dpmpp_2m", 1)])
@pytest.mark.parametrize("n", [3, 20])
def test_constant_data_prediction_is_reproduced_from_pure_noise(lib, kind, hist, n):
    """The model's v encodes the same x0 = c at every step, v = (alpha_t x - c) / sigma_t (at the terminal step: v = -c, whatever x is).
    Every step of a consistent solver lands on alpha_p c + (sigma_p / sigma_t)(x - alpha_t c) and the last one on c, from pure noise at
    t = N - 1, to float64 rounding: the bounds of test_sampler_cpu.test_constant_data_prediction_is_reproduced (1e-12 of the scale of
    the step's terms; here no term is divided by alpha_t, v is (|x| + |c|) / sigma_t at most)."""
    tab = c_table(lib, N_TRAIN, 1).astype(np.float64)
    c = randn(930, 4, 8, 8).astype(np.float64)
    x = randn(931, 4, 8, 8).astype(np.float64)
    h = None
    for i in range(n):
        t, tp, al, sg, c_x, c_v, c_h, c_n = c_ex(lib, kind, 0.0, "trailing", n, i, hist and h is not None, V, 1)
        assert c_n == 0.0 and (i > 0 or (t == N_TRAIN - 1 and al == 0.0))
        v = (al * x - c) / sg
        a_p = tab[int(tp)] if tp >= 0 else 1.0
        want = np.sqrt(a_p) * c + np.sqrt(1 - a_p) / sg * (x - al * c)
        new = c_x * x + c_v * v + (c_h * h if h is not None else 0.0)
        scale = (np.abs(x).max() + np.abs(c).max()) / sg
        assert np.abs(new - want).max() <= 1e-12 * scale, (kind, n, i)
        h = al * x - sg * v                          # the data prediction the v kernel keeps: c up to rounding
        assert np.abs(h - c).max() <= 1e-12 * scale
        x = new
    assert np.abs(x - c).max() <= 1e-12 * (np.abs(c).max() + 1.0)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_combinations_and_unknown_enums(lib):
    out = (C.c_double * 8)()
    for kind in KINDS:
        assert c_ex(lib, kind, 0.0, "trailing", 20, 0, 0, EPS, 1, raw=True) == -1       # eps + zero terminal SNR + trailing
        assert c_ex(lib, kind, 0.0, "trailing", 20, 5, 0, EPS, 1, raw=True) == -1       # ... at any step of such a list
        assert b"alpha_bar = 0" in lib.tsd_last_error()
        assert c_ex(lib, kind, 0.0, "leading", 20, 0, 0, EPS, 1, raw=True) == 0         # leading never reaches N - 1
        assert c_ex(lib, kind, 0.0, "trailing", 20, 0, 0, EPS, 1, start=1, raw=True) == 0   # img2img drops it
        assert c_ex(lib, kind, 0.0, "trailing", 20, 0, 0, V, 1, raw=True) == 0
    for pred, z in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert c_ex(lib, "ddim", 0.0, "leading", 20, 0, 0, pred, z, raw=True) == -1, (pred, z)
    assert lib.tsd_sampler_coeffs_ex(3, 0.0, 0, 1000, 5, 0, 0, 0, V, 0, out) == -1      # kind
    assert lib.tsd_sampler_coeffs_ex(1, -0.5, 0, 1000, 5, 0, 0, 0, V, 0, out) == -1     # eta < 0
    assert lib.tsd_sampler_coeffs_ex(1, 0.0, 0, 1000, 5, 0, 5, 0, V, 0, out) == -1      # step out of range
    assert lib.tsd_sampler_coeffs_ex(1, 0.0, 0, 1000, 5, 0, 0, 0, V, 0, None) == -1


# ---- 7. the Python side ---------------------------------------------------------------------------------------------------------------
def test_python_mirrors_return_what_the_library_returns(lib, tsd_mod):
    n = 20
    assert tsd_mod.alphas_cumprod(N_TRAIN, False).tobytes() == c_table(lib, N_TRAIN, 0).tobytes()
    assert tsd_mod.alphas_cumprod(N_TRAIN, True).tobytes() == c_table(lib, N_TRAIN, 1).tobytes()
    for pred, ztsnr, spacing in (("v", True, "trailing"), ("v", False, "leading"), ("epsilon", True, "leading")):
        for kind, eta, make in (("ddim", 0.5, lambda: tsd_mod.DDIMSampler(N_TRAIN, 0.5, spacing, prediction=pred, zero_terminal_snr=ztsnr)),
                                ("dpmpp_2m", 0.0, lambda: tsd_mod.DPMSolverMultistepSampler(N_TRAIN, spacing, prediction=pred,
                                                                                             zero_terminal_snr=ztsnr))):
            for strength in (None, 0.6):
                m = make()
                m.set_inference_timesteps(n)
                if strength:
                    m.set_strength(strength)
                assert m.alphas_cumprod.tobytes() == c_table(lib, N_TRAIN, ztsnr).tobytes()
                for i in range(len(m.timesteps)):
                    for hist in (0, 1):
                        want = c_ex(lib, kind, eta, spacing, n, i, hist, tsd_mod._lib.PREDICTION_TYPES[pred], ztsnr, start=m.start_step)
                        assert np.array_equal(np.array(m.coefficients(i, bool(hist)), dtype=np.float64), want)
    m = tsd_mod.DDIMSampler(N_TRAIN, 0.0, "trailing", prediction="v_prediction", zero_terminal_snr=True)
    m.set_inference_timesteps(4)
    x, v = randn(940, 4, 8, 8), randn(941, 4, 8, 8)
    new, x0 = m.step(0, x, v)
    assert np.array_equal(x0, -v.astype(np.float64))                           # the terminal step: alpha_t = 0, sigma_t = 1
    _, _, al, sg, c_x, c_v, _, _ = m.coefficients(1)
    new, x0 = m.step(1, x, v)
    assert np.array_equal(x0, al * x.astype(np.float64) - sg * v.astype(np.float64))
    refused = tsd_mod.DDIMSampler(N_TRAIN, 0.0, "trailing", zero_terminal_snr=True)   # epsilon on a list that holds abar = 0
    refused.set_inference_timesteps(4)
    with pytest.raises(tsd_mod.TsdError):
        refused.coefficients(1)
    with pytest.raises(ValueError):
        tsd_mod.DDIMSampler(N_TRAIN, prediction="sample")
    # the defaults are the float64 restatement they always were
    d = tsd_mod.DDIMSampler(N_TRAIN)
    assert d.prediction == "epsilon" and d.zero_terminal_snr is False and not d._ex


def test_read_scheduler_config(tsd_mod, tmp_path):
    import json
    from tsd import checkpoint
    got = checkpoint.read_scheduler_config(os.path.join(GOLDEN, "scheduler_config_v_ztsnr.json"))
    assert got == {"prediction": "v", "zero_terminal_snr": True, "spacing": "trailing", "num_training_steps": 1000}
    assert set(got) <= set(inspect.signature(tsd_mod.generate).parameters)     # they ARE generate's keywords
    assert set(got) - {"num_training_steps"} <= set(inspect.signature(tsd_mod.generate_stream).parameters)
    base = json.load(open(os.path.join(GOLDEN, "scheduler_config_v_ztsnr.json")))

    def write(**kw):
        p = tmp_path / "scheduler_config.json"
        p.write_text(json.dumps({k: v for k, v in dict(base, **kw).items() if v != "__drop__"}))
        return str(p)

    for bad in (dict(beta_schedule="squaredcos_cap_v2"), dict(beta_schedule="linear"), dict(beta_start=0.0001), dict(beta_end=0.02),
                dict(prediction_type="sample"), dict(timestep_spacing="linspace"), dict(trained_betas=[0.1, 0.2]),
                dict(num_train_timesteps=0)):
        with pytest.raises(ValueError):
            checkpoint.read_scheduler_config(write(**bad))
    # missing keys take diffusers' defaults: an SD-1.x config
    assert checkpoint.read_scheduler_config(write(prediction_type="__drop__", rescale_betas_zero_snr="__drop__", timestep_spacing="__drop__")) == \
        {"prediction": "epsilon", "zero_terminal_snr": False, "spacing": "leading", "num_training_steps": 1000}


def test_generate_defaults_are_unchanged(tsd_mod):
    for fn in (tsd_mod.generate, tsd_mod.generate_stream):
        p = inspect.signature(fn).parameters
        assert (p["prediction"].default, p["zero_terminal_snr"].default) == ("epsilon", False)
        assert (p["sampler"].default, p["eta"].default, p["spacing"].default) == ("ddpm", 0.0, "leading")
    p = inspect.signature(tsd_mod.Session.set_prediction).parameters
    assert (p["prediction"].default, p["zero_terminal_snr"].default) == ("epsilon", False)
    from tsd import _lib
    assert _lib.PREDICTION_TYPES == {"epsilon": EPS, "v": V}
    assert _lib.prediction_type("v_prediction") == V and _lib.prediction_type("V") == V and _lib.prediction_type("sample") == -1
    assert "prediction" not in tsd_mod.Request._fields and "zero_terminal_snr" not in tsd_mod.Request._fields   # session-wide, not per request


def test_header_python_and_mojo_name_every_new_symbol(tsd_mod):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    new = ["tsd_sampler_alphas_cumprod", "tsd_sampler_coeffs_ex", "tsd_sampler_step_v_f32", "tsd_session_set_prediction",
           "tsd_session_prediction"]
    declared = tsd_mod._lib.declared_symbols()
    shim = open(os.path.join(root, "stable-diffusion.mojo_amd", "mojo_shim", "tsd_ffi.mojo")).read()
    lib = tsd_mod._lib.lib()
    for name in new:
        assert name in declared and f'"{name}"' in shim and getattr(lib, name).argtypes is not None, name
    dshim = open(os.path.join(root, "stable-diffusion.mojo_amd", "mojo_shim", "diffusion_shim.mojo")).read()
    assert "fn sampler_step_v(" in dshim and "fn set_prediction(" in dshim
    hdr = open(os.path.join(root, "include", "tsd.h")).read()
    assert "TSD_PRED_EPSILON = 0, TSD_PRED_V = 1" in hdr and "rescale_zero_terminal_snr" in hdr   # the note on diffusers' last bits
