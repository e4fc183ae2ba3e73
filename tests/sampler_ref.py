"""fp64 restatement of the published sampler updates (test infrastructure, shared by test_sampler_cpu.py and test_gpu_sampler.py).
Each update is a FUNCTION of (x, eps, previous data prediction, noise) in the form its paper prints; its linear coefficients are read
off by probing it with unit inputs, nothing is expanded by hand."""
import numpy as np

from oracle import sampler as osampler

N_TRAIN = 1000


class Papers:
    """The three updates as functions, in the form the papers print them, on the fp32 alphas_cumprod table the reference builds
    (taken from the oracle, sampler.mojo:28-32) promoted to fp64.  `ts` is the timestep list; the step after the last is abar = 1."""

    def __init__(self, ts, n_train=N_TRAIN):
        self.ab = osampler.DDPMSampler(n_train).alphas_cumprod.astype(np.float64)
        self.ts = [int(t) for t in ts]

    def abar(self, i):
        return self.ab[self.ts[i]] if 0 <= i < len(self.ts) else 1.0

    def ddpm(self, i, x, eps, x0_prev, z):
        """Ho et al. 2020, eq. 6-7 (+ eq. 15 for x0): q(x_{t-1} | x_t, x0) with mean and variance of eq. 7; the reference's clamp of the
        variance at 1e-20 and no noise on the step onto the clean sample (sampler.mojo:53-65, :99-105)."""
        a_t, a_p = self.abar(i), self.abar(i + 1)
        x0 = (x - np.sqrt(1 - a_t) * eps) / np.sqrt(a_t)
        alpha_step = a_t / a_p
        beta_step = 1 - alpha_step
        mean = np.sqrt(a_p) * beta_step / (1 - a_t) * x0 + np.sqrt(alpha_step) * (1 - a_p) / (1 - a_t) * x
        var = max((1 - a_p) / (1 - a_t) * beta_step, 1e-20)
        return mean + (np.sqrt(var) * z if i + 1 < len(self.ts) else 0.0)

    def ddim(self, eta):
        def f(i, x, eps, x0_prev, z):
            """Song et al. 2021, eq. 12 with sigma_t(eta) of eq. 16."""
            a_t, a_p = self.abar(i), self.abar(i + 1)
            sigma = eta * np.sqrt((1 - a_p) / (1 - a_t)) * np.sqrt(1 - a_t / a_p)
            x0 = (x - np.sqrt(1 - a_t) * eps) / np.sqrt(a_t)
            return np.sqrt(a_p) * x0 + np.sqrt(max(1 - a_p - sigma ** 2, 0.0)) * eps + sigma * z
        return f

    def dpmpp_2m(self, i, x, eps, x0_prev, z):
        """Lu et al. 2022, algorithm 2 (data prediction): x0_prev is None without history (first order, also on the first step);
        the step onto the clean sample (sigma = 0, lambda infinite) returns the data prediction."""
        a_t, a_p = self.abar(i), self.abar(i + 1)
        al_t, sg_t, al_p, sg_p = np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)
        x0 = (x - sg_t * eps) / al_t
        if sg_p == 0.0:
            return x0
        lam_t, lam_p = np.log(al_t / sg_t), np.log(al_p / sg_p)
        h = lam_p - lam_t
        D = x0
        if x0_prev is not None and i > 0:
            a_l = self.abar(i - 1)
            r = (lam_t - np.log(np.sqrt(a_l) / np.sqrt(1 - a_l))) / h
            D = (1 + 1 / (2 * r)) * x0 - 1 / (2 * r) * x0_prev
        return sg_p / sg_t * x - al_p * (np.exp(-h) - 1) * D

    def linear_form(self, update, i, have_history):
        """(alpha_t, sigma_t, c_x, c_e, c_h, c_n) of an update that is linear in (x, eps, x0_prev, z): probe it with unit inputs."""
        hp = (lambda v: v) if have_history else (lambda v: None)
        a_t = self.abar(i)
        return np.array([np.sqrt(a_t), np.sqrt(1 - a_t), update(i, 1.0, 0.0, hp(0.0), 0.0), update(i, 0.0, 1.0, hp(0.0), 0.0),
                         update(i, 0.0, 0.0, hp(1.0), 0.0) if have_history else 0.0, update(i, 0.0, 0.0, hp(0.0), 1.0)])
