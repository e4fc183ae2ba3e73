"""Host-side mirror of `sampler.mojo` (DDPMSampler).  The schedule scalars are host code exactly as in the
reference (a few fp32 scalars per step); the per-step tensor update runs on the GPU inside the
session (`tsd_session_step`: fused CFG combine + posterior mean + noise, SURVEY.md App.D K9).
DDIMSampler and DPMSolverMultistepSampler have no reference counterpart: they mirror the samplers `Session.set_sampler` selects."""
import numpy as np


class DDPMSampler:
    """`DDPMSampler` sampler.mojo:5-124 (num_training_steps is a parameter: App.A D22)."""

    def __init__(self, seed_val=0, num_training_steps=1000, beta_start=0.00085, beta_end=0.0120):
        self.seed_val = seed_val
        self.num_training_steps = num_training_steps
        self.betas = (np.linspace(np.float32(beta_start) ** 0.5, np.float32(beta_end) ** 0.5, num_training_steps,
                                  dtype=np.float32) ** 2).astype(np.float32)          # :28-30
        self.alphas = (1.0 - self.betas).astype(np.float32)                           # :31
        self.alphas_cumprod = np.cumprod(self.alphas, dtype=np.float32)               # :32
        self.timesteps = np.arange(num_training_steps)[::-1].copy()                  # :33
        self.num_inference_steps = 1
        self.start_step = 0

    def set_inference_timesteps(self, num_inference_steps=1):                         # :35-44
        self.num_inference_steps = num_inference_steps
        ratio = self.num_training_steps // num_inference_steps
        self.timesteps = np.round(np.arange(num_inference_steps)[::-1] * ratio).astype(np.int64)

    def get_previous_timestep(self, timestep):                                        # :46-51
        return timestep - self.num_training_steps // self.num_inference_steps

    def get_variance(self, timestep):                                                 # :53-65
        prev = self.get_previous_timestep(timestep)
        a_t = np.float32(self.alphas_cumprod[timestep])
        a_prev = np.float32(self.alphas_cumprod[prev]) if prev >= 0 else np.float32(1.0)
        cur_beta = np.float32(1.0) - a_t / a_prev
        var = (np.float32(1.0) - a_prev) / (np.float32(1.0) - a_t) * cur_beta
        return np.float32(max(var, np.float32(1e-20)))

    def set_strength(self, strength):                                                 # :67-73 (intended slice, App.A D21)
        start = self.num_inference_steps - int(self.num_inference_steps * strength)
        self.timesteps = self.timesteps[start:]
        self.start_step = start


class _LinearMultistepSampler(DDPMSampler):
    """Host mirror of the samplers the device session runs through `k_sampler_step` (include/tsd.h "samplers"):
    x' = c_x x + c_e e + c_h h + c_n z with x0 = (x - sigma_t e) / alpha_t and h the previous step's x0.  The scalars are
    restated here in float64 on the same fp32 alphas_cumprod table; `tsd_sampler_coeffs` is the implementation the session uses.

    prediction "v" (the model output means v = alpha e - sigma x0: x0 = alpha_t x - sigma_t v, and c_e multiplies v) and
    zero_terminal_snr=True (the rescaled table of `tsd.alphas_cumprod`) mirror `Session.set_prediction`.  With either, the table and the
    scalars are the library's own (`tsd_sampler_alphas_cumprod`, `tsd_sampler_coeffs_ex`; host code, no GPU), not a restatement: the
    restatement of the v rows is tests/vpred_ref.py."""
    KIND = None  # tsd_sampler_kind of the subclass

    def __init__(self, num_training_steps=1000, spacing="leading", prediction="epsilon", zero_terminal_snr=False, **kw):
        super().__init__(num_training_steps=num_training_steps, **kw)
        if spacing not in ("leading", "trailing"):
            raise ValueError(f"spacing must be 'leading' or 'trailing', got {spacing!r}")
        if prediction == "v_prediction":
            prediction = "v"
        if prediction not in ("epsilon", "v"):
            raise ValueError(f"prediction must be 'epsilon' or 'v', got {prediction!r}")
        self.spacing = spacing
        self.prediction = prediction
        self.zero_terminal_snr = bool(zero_terminal_snr)
        self._ex = prediction != "epsilon" or self.zero_terminal_snr
        if self._ex:
            if kw.get("beta_start", 0.00085) != 0.00085 or kw.get("beta_end", 0.0120) != 0.0120:
                raise ValueError("prediction / zero_terminal_snr run on the library's table: beta_start and beta_end must be the defaults")
            from .utils import alphas_cumprod
            self.alphas_cumprod = alphas_cumprod(num_training_steps, self.zero_terminal_snr)

    def _coefficients_ex(self, i, have_history, eta=0.0):
        """The out[8] of `tsd_sampler_coeffs_ex` for this sampler's schedule, prediction type and table."""
        import ctypes as C
        from ._lib import PREDICTION_TYPES, TIMESTEP_SPACINGS, check, lib
        out = (C.c_double * 8)()
        check(lib().tsd_sampler_coeffs_ex(self.KIND, float(eta), TIMESTEP_SPACINGS[self.spacing], self.num_training_steps,
                                          self.num_inference_steps, self.start_step, int(i), 1 if have_history else 0,
                                          PREDICTION_TYPES[self.prediction], 1 if self.zero_terminal_snr else 0, out))
        t, tp = int(out[0]), int(out[1])
        return (t, tp) + tuple(float(v) for v in out[2:])

    def set_inference_timesteps(self, num_inference_steps=1):
        if self.spacing == "leading":
            return super().set_inference_timesteps(num_inference_steps)
        self.num_inference_steps = num_inference_steps
        N = self.num_training_steps                         # round(N - k N/n) - 1: starts at N - 1 (halves to even)
        self.timesteps = np.round(N - np.arange(num_inference_steps) * (N / num_inference_steps)).astype(np.int64) - 1

    def _step_scalars(self, i):
        """(t, t_prev, abar_t, abar_prev): the previous timestep of step i is the next entry; then the clean sample (abar = 1)."""
        t = int(self.timesteps[i])
        tp = int(self.timesteps[i + 1]) if i + 1 < len(self.timesteps) else -1
        return t, tp, float(self.alphas_cumprod[t]), float(self.alphas_cumprod[tp]) if tp >= 0 else 1.0

    def coefficients(self, i, have_history=False):
        """-> (t, t_prev, alpha_t, sigma_t, c_x, c_e, c_h, c_n), the out[8] of `tsd_sampler_coeffs`."""
        raise NotImplementedError

    def step(self, i, latents, model_output, history=None, noise=None):
        """One update in float64 -> (x', x0); `history` is the x0 the previous step returned (None: first order)."""
        _, _, al, sg, c_x, c_e, c_h, c_n = self.coefficients(i, history is not None)
        x, e = np.asarray(latents, dtype=np.float64), np.asarray(model_output, dtype=np.float64)
        out = c_x * x + c_e * e
        if history is not None:
            out = out + c_h * np.asarray(history, dtype=np.float64)
        if noise is not None:
            out = out + c_n * np.asarray(noise, dtype=np.float64)
        return out, (al * x - sg * e) if self.prediction == "v" else (x - sg * e) / al


class DDIMSampler(_LinearMultistepSampler):
    """DDIM (Song et al. 2021, eq. 12; sigma = eta * eq. 16).  eta = 0 is deterministic, eta = 1 is the DDPM posterior."""

    KIND = 1

    def __init__(self, num_training_steps=1000, eta=0.0, spacing="leading", **kw):
        super().__init__(num_training_steps, spacing, **kw)
        self.eta = float(eta)

    def coefficients(self, i, have_history=False):
        if self._ex:
            return self._coefficients_ex(i, have_history, self.eta)
        t, tp, a_t, a_p = self._step_scalars(i)
        var = self.eta ** 2 * (1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p)
        c_x = np.sqrt(a_p / a_t)
        c_e = np.sqrt(max(1.0 - a_p - var, 0.0)) - c_x * np.sqrt(1.0 - a_t)
        return t, tp, np.sqrt(a_t), np.sqrt(1.0 - a_t), c_x, c_e, 0.0, np.sqrt(var)


class DPMSolverMultistepSampler(_LinearMultistepSampler):
    """DPM-Solver++(2M) (Lu et al. 2022, algorithm 2, data prediction): second order from the previous step's x0; first order on
    the first step, on the step onto the clean sample and without history.  Deterministic (c_n = 0)."""
    KIND = 2

    def coefficients(self, i, have_history=False):
        if self._ex:
            return self._coefficients_ex(i, have_history)
        t, tp, a_t, a_p = self._step_scalars(i)
        al, sg = np.sqrt(a_t), np.sqrt(1.0 - a_t)
        if tp < 0:                                          # lambda_prev is infinite: x' = x0
            return t, tp, al, sg, 1.0 / al, -sg / al, 0.0, 0.0
        lam = lambda a: 0.5 * np.log(a / (1.0 - a))  # noqa: E731
        h = lam(a_p) - lam(a_t)
        g = -np.sqrt(a_p) * np.expm1(-h)                    # x' = (sigma_prev / sigma_t) x + g D
        w1 = 0.0
        if have_history and i > 0:                          # D = (1 + 1/(2r)) x0 - 1/(2r) x0_prev, r = h_prev / h
            r = (lam(a_t) - lam(float(self.alphas_cumprod[int(self.timesteps[i - 1])]))) / h
            w1 = 1.0 / (2.0 * r)
        w0 = 1.0 + w1
        return t, tp, al, sg, np.sqrt(1.0 - a_p) / sg + g * w0 / al, -g * w0 * sg / al, -g * w1, 0.0
