"""fp64 restatement of the zero-terminal-SNR table and of the three sampler updates for a v-prediction model (test infrastructure,
shared by test_vpred_cpu.py and test_gpu_vpred.py), written from the papers and independently of csrc/sampler.cpp:
  - Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", algorithm 1, on the oracle's fp32 table;
  - v = alpha eps - sigma x0 (Salimans & Ho 2022), hence x0 = alpha x - sigma v and eps = sigma x + alpha v, substituted into the
    updates in the form their papers print them (Ho et al. 2020 eq. 7; Song et al. 2021 eq. 12, 16; Lu et al. 2022 algorithm 2).
Each update is a FUNCTION of (x, v, previous data prediction, noise); its linear coefficients are read off by probing it with unit
inputs, nothing is expanded by hand.  e^-h of DPM-Solver++ is written as the ratio (sigma_p / alpha_p) (alpha_t / sigma_t) it is, not
through log and exp: finite (zero) at alpha_t = 0, and no algebra shared with the library's expm1 form.

`Err` is a running error analysis: a double with a bound on its distance from the real-arithmetic value of the expression that made it,
one rounding (2^-53 relative) per operation plus what the operands' own errors do to the result, first order with the second-order
product term kept.  Evaluating a restatement on Err numbers gives the forward error bound of that expression without anyone choosing a
constant: the test holds |library - restatement| to the sum of both sides' bounds."""
import math

import numpy as np

from oracle import sampler as osampler

N_TRAIN = 1000
U = 2.0 ** -53


class Err:
    """value +- err, where err bounds |value - exact| for the expression evaluated so far (inputs are exact)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def _r(self, v, e):                     # one rounding of the result on top of the propagated error
        return Err(v, e + U * abs(v))

    def __add__(self, o):
        o = Err.of(o)
        return self._r(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Err.of(o) - self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.of(o)
        return self._r(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        q = self.v / o.v
        lo = abs(o.v) - o.e
        assert lo > 0.0, "division by a quantity whose error bound reaches zero"
        return self._r(q, (self.e + abs(q) * o.e) / lo)

    def __rtruediv__(self, o):
        return Err.of(o) / self

    def sqrt(self):
        r = math.sqrt(max(self.v, 0.0))
        lo = self.v - self.e
        # the exact argument lies in [a - e, a + e]: sqrt(a) - sqrt(a - e) = e / (sqrt(a) + sqrt(a - e)) is the larger side
        prop = self.e / (math.sqrt(lo) + r) if lo > 0.0 else math.sqrt(max(self.v, 0.0) + self.e)
        return self._r(r, prop)

    def log(self):
        lo = self.v - self.e
        assert lo > 0.0
        r = math.log(self.v)
        return Err(r, self.e / lo + 2.0 * U * abs(r) + U)   # libm: under one ulp of the result; the argument's relative error adds as is

    def expm1(self):
        r = math.expm1(self.v)
        return Err(r, math.exp(self.v + self.e) * self.e + 2.0 * U * abs(r))

    def maxc(self, c):
        """max(self, c) for an exact constant c: the bound carries over (max is 1-Lipschitz)."""
        return Err(max(self.v, c), self.e)

    def __float__(self):
        return self.v


def sqrt(x):
    return x.sqrt() if isinstance(x, Err) else np.sqrt(x)


def log(x):
    return x.log() if isinstance(x, Err) else np.log(x)


def expm1(x):
    return x.expm1() if isinstance(x, Err) else np.expm1(x)


def maxc(x, c):
    return x.maxc(c) if isinstance(x, Err) else max(x, c)


def val(x):
    return x.v if isinstance(x, Err) else float(x)


def plain_table(n_train=N_TRAIN):
    """The reference's fp32 alphas_cumprod (sampler.mojo:28-32), from the oracle."""
    return osampler.DDPMSampler(n_train).alphas_cumprod.astype(np.float32)


def zero_terminal_snr_table64(n_train=N_TRAIN):
    """Lin et al. 2023, algorithm 1, in float64 on the fp32 table: alphas_bar_sqrt -= its last entry (the terminal SNR becomes zero), then
    *= first / (first - last) (the first entry keeps its value); squared.  Not rounded to float."""
    s = np.sqrt(plain_table(n_train).astype(np.float64))
    s0, sT = s[0], s[-1]
    s = (s - sT) * (s0 / (s0 - sT))
    return s * s


def table(n_train=N_TRAIN, zero_terminal_snr=False):
    """The table a session of that choice runs on, as float32 (the restatement's own rounding of algorithm 1)."""
    return zero_terminal_snr_table64(n_train).astype(np.float32) if zero_terminal_snr else plain_table(n_train)


class VPapers:
    """The three updates for a model output v, on a given fp32 table `ab` (promoted to fp64) and timestep list `ts`; the step after the
    last is abar = 1.  track=True: the table entries are Err numbers and every coefficient comes with its forward error bound."""

    def __init__(self, ts, ab, track=False):
        self.ab = [Err(float(a)) if track else float(a) for a in np.asarray(ab, dtype=np.float64)]
        self.ts = [int(t) for t in ts]
        self.one = Err(1.0) if track else 1.0

    def abar(self, i):
        return self.ab[self.ts[i]] if 0 <= i < len(self.ts) else self.one

    def alpha_sigma(self, i):
        a = self.abar(i)
        return sqrt(a), sqrt(1.0 - a)

    def x0_eps(self, i, x, v):
        """Salimans & Ho 2022: v = alpha eps - sigma x0 with alpha^2 + sigma^2 = 1."""
        al, sg = self.alpha_sigma(i)
        return al * x - sg * v, sg * x + al * v

    def ddpm(self, i, x, v, x0_prev, z):
        """Ho et al. 2020, eq. 6-7: the posterior q(x_{t-1} | x_t, x0); variance clamped at 1e-20, no noise onto the clean sample."""
        a_t, a_p = self.abar(i), self.abar(i + 1)
        x0, _ = self.x0_eps(i, x, v)
        alpha_step = a_t / a_p
        beta_step = 1.0 - alpha_step
        mean = sqrt(a_p) * beta_step / (1.0 - a_t) * x0 + sqrt(alpha_step) * (1.0 - a_p) / (1.0 - a_t) * x
        var = maxc((1.0 - a_p) / (1.0 - a_t) * beta_step, 1e-20)
        return mean + (sqrt(var) * z if i + 1 < len(self.ts) else 0.0)

    def ddim(self, eta):
        def f(i, x, v, x0_prev, z):
            """Song et al. 2021, eq. 12 with sigma_t(eta)^2 of eq. 16."""
            a_t, a_p = self.abar(i), self.abar(i + 1)
            x0, eps = self.x0_eps(i, x, v)
            var = (eta * eta) * ((1.0 - a_p) / (1.0 - a_t)) * (1.0 - a_t / a_p)
            return sqrt(a_p) * x0 + sqrt(maxc(1.0 - a_p - var, 0.0)) * eps + sqrt(var) * z
        return f

    def dpmpp_2m(self, i, x, v, x0_prev, z):
        """Lu et al. 2022, algorithm 2 (data prediction): x' = (sigma_p / sigma_t) x - alpha_p (e^-h - 1) D with
        e^-h = (sigma_p / alpha_p) (alpha_t / sigma_t); D = x0 without history, on the first step and onto the clean sample, else
        (1 + 1/(2r)) x0 - 1/(2r) x0_prev with r = h_prev / h.  A previous step at abar = 0 has lambda = -inf: r = inf, 1/(2r) = 0."""
        al_t, sg_t = self.alpha_sigma(i)
        al_p, sg_p = self.alpha_sigma(i + 1)
        x0, _ = self.x0_eps(i, x, v)
        if i + 1 >= len(self.ts):
            return x0
        emh = (sg_p / al_p) * (al_t / sg_t)
        D = x0
        if x0_prev is not None and i > 0 and val(self.abar(i - 1)) > 0.0:
            al_l, sg_l = self.alpha_sigma(i - 1)
            lam_t, lam_p, lam_l = log(al_t / sg_t), log(al_p / sg_p), log(al_l / sg_l)
            r = (lam_t - lam_l) / (lam_p - lam_t)
            D = (1.0 + 1.0 / (2.0 * r)) * x0 - 1.0 / (2.0 * r) * x0_prev
        return sg_p / sg_t * x - al_p * (emh - 1.0) * D

    def update(self, kind, eta=0.0):
        return {"ddpm": self.ddpm, "ddim": self.ddim(eta), "dpmpp_2m": self.dpmpp_2m}[kind]

    def linear_form(self, update, i, have_history):
        """[alpha_t, sigma_t, c_x, c_v, c_h, c_n] of an update that is linear in (x, v, x0_prev, z): probe it with unit inputs."""
        hp = (lambda h: h) if have_history else (lambda h: None)
        al, sg = self.alpha_sigma(i)
        return [al, sg, update(i, 1.0, 0.0, hp(0.0), 0.0), update(i, 0.0, 1.0, hp(0.0), 0.0),
                update(i, 0.0, 0.0, hp(1.0), 0.0) if have_history else 0.0, update(i, 0.0, 0.0, hp(0.0), 1.0)]
