// sampler.cpp - host side of the denoise schedule: the alphas_cumprod table, the timestep lists and the per-step scalars of the
// samplers (no GPU).  The table is the reference's fp32 Tensor (sampler.mojo:28-32); everything derived from it here is computed in
// double and rounded to float once, where the kernel takes it (kernels_sampler.hip).  The session's DDPM path does not come through
// sampler_coeffs: it keeps the reference's fp32 scalars (ddpm_coeffs below) and its own kernel.  sampler_step_plan is the one place
// that turns a schedule index into what an update launch is given, for the lockstep step and for a slot alike (session.cpp).
// v-prediction (TSD_PRED_V) has rows of its own, sampler_coeffs_v, written without 1 / alpha_t, and a table of its own choice: the
// zero-terminal-SNR rescale of the same fp32 table (Lin et al. 2023, algorithm 1).
#include <math.h>

#include <algorithm>

#include "common.h"

void sampler_alphas_cumprod(int n_train, std::vector<float>& out) {
  // betas = linspace(sqrt(b0), sqrt(b1), N)^2 ; alphas_cumprod = cumprod(1 - betas)   (sampler.mojo:28-32), fp32
  const int N = n_train;
  out.resize(N);
  const float b0 = sqrtf(0.00085f), b1 = sqrtf(0.0120f);
  float prod = 1.f;
  for (int i = 0; i < N; i++) {
    const float step = N > 1 ? (b1 - b0) / (float)(N - 1) : 0.f;  // numpy.linspace order: i*step + start
    const float v = (float)i * step + b0;
    const float beta = v * v;
    prod *= (1.f - beta);
    out[i] = prod;
  }
}

int sampler_alphas_cumprod(int n_train, int zero_terminal_snr, std::vector<float>& out) {
  if (zero_terminal_snr != 0 && zero_terminal_snr != 1) TSD_FAIL(TSD_E_ARG, "schedule: zero_terminal_snr %d (0 or 1)", zero_terminal_snr);
  sampler_alphas_cumprod(n_train, out);
  if (!zero_terminal_snr) return TSD_OK;
  // Lin et al. 2023, algorithm 1 on s = sqrt(abar): shift so that the last entry is 0, scale so that the first keeps its value.  In double
  // from the fp32 table, ONE rounding to float per entry (diffusers goes back through fp32 betas and a cumprod: the last bits differ).
  const int N = n_train;
  if (N < 2) TSD_FAIL(TSD_E_ARG, "schedule: a zero-terminal-SNR table needs at least 2 training steps (train=%d)", N);
  const double s0 = sqrt((double)out[0]), sT = sqrt((double)out[N - 1]);
  for (int i = 0; i < N - 1; i++) {
    const double si = (sqrt((double)out[i]) - sT) * s0 / (s0 - sT);
    out[i] = (float)(si * si);
  }
  out[N - 1] = 0.f;  // (sT - sT) * ... : exactly zero, stated rather than computed
  return TSD_OK;
}

int sampler_timesteps(int spacing, int n_train, int n_infer, int start_step, std::vector<int>& out) {
  if (n_train <= 0 || n_infer <= 0 || n_infer > n_train || start_step < 0 || start_step >= n_infer)
    TSD_FAIL(TSD_E_ARG, "schedule: train=%d infer=%d start=%d", n_train, n_infer, start_step);
  out.clear();
  if (spacing == TSD_SPACING_LEADING) {
    // timesteps = round(arange(n)[::-1] * (N // n))  (sampler.mojo:40-43)
    const int ratio = n_train / n_infer;
    for (int i = n_infer - 1; i >= 0; i--) out.push_back(i * ratio);
  } else if (spacing == TSD_SPACING_TRAILING) {
    // timesteps = round(N - k N/n) - 1, k = 0..n-1 (halves to even, as numpy rounds): starts at N-1, the last step leaves N/n - 1
    const double step = (double)n_train / (double)n_infer;
    for (int k = 0; k < n_infer; k++) out.push_back((int)nearbyint((double)n_train - (double)k * step) - 1);
  } else {
    TSD_FAIL(TSD_E_ARG, "schedule: timestep spacing %d (0 leading, 1 trailing)", spacing);
  }
  // then drop `start_step` (set_strength, App.A D21)
  out.erase(out.begin(), out.begin() + start_step);
  return TSD_OK;
}

int sampler_coeffs(int kind, double eta, const std::vector<float>& ac, const std::vector<int>& ts, int i, int have_history,
                   double out[8]) {
  if (i < 0 || i >= (int)ts.size()) TSD_FAIL(TSD_E_ARG, "sampler: step %d out of range (%d steps)", i, (int)ts.size());
  if (!(eta >= 0.0)) TSD_FAIL(TSD_E_ARG, "sampler: eta %g < 0", eta);
  // the previous timestep of step i is the next entry of the list; after the last entry comes the clean sample (alpha_bar = 1)
  const int t = ts[i], tp = i + 1 < (int)ts.size() ? ts[i + 1] : -1;
  const double a_t = ac[t], a_p = tp >= 0 ? (double)ac[tp] : 1.0;
  const double alpha_t = sqrt(a_t), sigma_t = sqrt(1.0 - a_t), alpha_p = sqrt(a_p), sigma_p = sqrt(1.0 - a_p);
  double c_x = 0, c_e = 0, c_h = 0, c_n = 0;
  if (kind == TSD_SAMPLER_DDPM) {
    // Ho et al. 2020, eq. 7 with x0 = (x - sigma_t e) / alpha_t substituted: the posterior mean c_x0 x0 + c_xt x and its variance
    const double cur_a = a_t / a_p, cur_b = 1.0 - cur_a;
    const double c_x0 = alpha_p * cur_b / (1.0 - a_t), c_xt = sqrt(cur_a) * (1.0 - a_p) / (1.0 - a_t);
    c_x = c_xt + c_x0 / alpha_t;
    c_e = -c_x0 * sigma_t / alpha_t;
    c_n = tp >= 0 ? sqrt(std::max((1.0 - a_p) / (1.0 - a_t) * cur_b, 1e-20)) : 0.0;
  } else if (kind == TSD_SAMPLER_DDIM) {
    // Song et al. 2021, eq. 12 with sigma of eq. 16: x' = alpha_p x0 + sqrt(1 - a_p - sigma^2) e + sigma z
    const double var = eta * eta * (1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p);
    c_x = sqrt(a_p / a_t);
    c_e = sqrt(std::max(1.0 - a_p - var, 0.0)) - c_x * sigma_t;
    c_n = sqrt(var);
  } else if (kind == TSD_SAMPLER_DPMPP_2M) {
    // Lu et al. 2022, alg. 2: x' = (sigma_p / sigma_t) x - alpha_p (e^-h - 1) D, h = lambda_p - lambda_t, lambda = log(alpha / sigma)
    if (tp < 0) {  // onto the clean sample: lambda_p is infinite, e^-h = 0 and sigma_p = 0, i.e. x' = x0
      c_x = 1.0 / alpha_t;
      c_e = -sigma_t / alpha_t;
    } else {
      const double lam_t = 0.5 * log(a_t / (1.0 - a_t)), lam_p = 0.5 * log(a_p / (1.0 - a_p));
      const double h = lam_p - lam_t;
      const double g = -alpha_p * expm1(-h);  // x' = (sigma_p / sigma_t) x + g D
      double w0 = 1.0, w1 = 0.0;              // D = w0 x0 - w1 x0_prev
      if (have_history && i > 0) {            // D = (1 + 1/(2r)) x0 - 1/(2r) x0_prev, r = h_prev / h
        const double a_l = ac[ts[i - 1]];
        const double r = (lam_t - 0.5 * log(a_l / (1.0 - a_l))) / h;
        w1 = 1.0 / (2.0 * r);
        w0 = 1.0 + w1;
      }
      c_x = sigma_p / sigma_t + g * w0 / alpha_t;
      c_e = -g * w0 * sigma_t / alpha_t;
      c_h = -g * w1;
    }
  } else {
    TSD_FAIL(TSD_E_ARG, "sampler: kind %d (0 DDPM, 1 DDIM, 2 DPM-Solver++(2M))", kind);
  }
  out[0] = t; out[1] = tp; out[2] = alpha_t; out[3] = sigma_t;
  out[4] = c_x; out[5] = c_e; out[6] = c_h; out[7] = c_n;
  return TSD_OK;
}

// The same three rows for a model output that means v = alpha e - sigma x0 (Salimans & Ho 2022): x0 = alpha x - sigma v and
// e = sigma x + alpha v substituted into the papers' equations, so nothing divides by alpha_t and every row is finite on the terminal
// step of a zero-terminal-SNR table (abar_t = 0: alpha_t = 0, sigma_t = 1, x0 = -v).  out[5] multiplies v.
static int sampler_coeffs_v(int kind, double eta, const std::vector<float>& ac, const std::vector<int>& ts, int i, int have_history,
                            double out[8]) {
  if (i < 0 || i >= (int)ts.size()) TSD_FAIL(TSD_E_ARG, "sampler: step %d out of range (%d steps)", i, (int)ts.size());
  if (!(eta >= 0.0)) TSD_FAIL(TSD_E_ARG, "sampler: eta %g < 0", eta);
  const int t = ts[i], tp = i + 1 < (int)ts.size() ? ts[i + 1] : -1;
  const double a_t = ac[t], a_p = tp >= 0 ? (double)ac[tp] : 1.0;  // a_p > a_t >= 0: the table decreases and the list descends
  const double alpha_t = sqrt(a_t), sigma_t = sqrt(1.0 - a_t), alpha_p = sqrt(a_p), sigma_p = sqrt(1.0 - a_p);
  double c_x = 0, c_v = 0, c_h = 0, c_n = 0;
  if (kind == TSD_SAMPLER_DDPM) {
    // Ho et al. 2020, eq. 7: c_x0 x0 + c_xt x.  At abar_t = 0: cur_a = 0, c_xt = 0, c_x0 = alpha_p - x' = alpha_p x0 + c_n z
    const double cur_a = a_t / a_p, cur_b = 1.0 - cur_a;
    const double c_x0 = alpha_p * cur_b / (1.0 - a_t), c_xt = sqrt(cur_a) * (1.0 - a_p) / (1.0 - a_t);
    c_x = c_xt + c_x0 * alpha_t;
    c_v = -c_x0 * sigma_t;
    c_n = tp >= 0 ? sqrt(std::max((1.0 - a_p) / (1.0 - a_t) * cur_b, 1e-20)) : 0.0;
  } else if (kind == TSD_SAMPLER_DDIM) {
    // Song et al. 2021, eq. 12: x' = alpha_p x0 + d e + sqrt(var) z.  At abar_t = 0 the variance of eq. 16 is eta^2 (1 - a_p).
    const double var = a_t > 0.0 ? eta * eta * (1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p) : eta * eta * (1.0 - a_p);
    const double d = sqrt(std::max(1.0 - a_p - var, 0.0));
    c_x = alpha_p * alpha_t + d * sigma_t;
    c_v = d * alpha_t - alpha_p * sigma_t;
    c_n = sqrt(var);
  } else if (kind == TSD_SAMPLER_DPMPP_2M) {
    // Lu et al. 2022, alg. 2: x' = (sigma_p / sigma_t) x + g D, g = -alpha_p expm1(-h), D = w0 x0 - w1 x0_prev
    if (tp < 0) {  // onto the clean sample: x' = x0
      c_x = alpha_t;
      c_v = -sigma_t;
    } else {
      double g, w0 = 1.0, w1 = 0.0;
      if (a_t > 0.0) {
        const double lam_t = 0.5 * log(a_t / (1.0 - a_t)), lam_p = 0.5 * log(a_p / (1.0 - a_p));
        const double h = lam_p - lam_t;
        g = -alpha_p * expm1(-h);
        // the step after a terminal one: lambda of the step before is -inf, r = +inf and 1/(2r) = 0 - first order, stated here
        const double a_l = have_history && i > 0 ? (double)ac[ts[i - 1]] : 0.0;
        if (a_l > 0.0) {
          const double r = (lam_t - 0.5 * log(a_l / (1.0 - a_l))) / h;
          w1 = 1.0 / (2.0 * r);
          w0 = 1.0 + w1;
        }
      } else {
        g = alpha_p;  // the terminal step: lambda_t = -inf, h = +inf, e^-h = 0 - the DDIM(0) step, and no step before it has a lambda
      }
      c_x = sigma_p / sigma_t + g * w0 * alpha_t;
      c_v = -g * w0 * sigma_t;
      c_h = w1 != 0.0 ? -g * w1 : 0.0;  // first order: +0, the DDIM row's
    }
  } else {
    TSD_FAIL(TSD_E_ARG, "sampler: kind %d (0 DDPM, 1 DDIM, 2 DPM-Solver++(2M))", kind);
  }
  out[0] = t; out[1] = tp; out[2] = alpha_t; out[3] = sigma_t;
  out[4] = c_x; out[5] = c_v; out[6] = c_h; out[7] = c_n;
  return TSD_OK;
}

int sampler_prediction_ok(int prediction, const std::vector<float>& ac, const std::vector<int>& ts) {
  if (prediction != TSD_PRED_EPSILON && prediction != TSD_PRED_V)
    TSD_FAIL(TSD_E_ARG, "sampler: prediction type %d (0 epsilon, 1 v)", prediction);
  if (prediction == TSD_PRED_EPSILON)
    for (int t : ts)
      if (!(ac[t] > 0.f))
        TSD_FAIL(TSD_E_ARG, "sampler: timestep %d of this list has alpha_bar = 0 (zero-terminal-SNR table): x0 = (x - sigma e) / alpha does "
                 "not exist there; epsilon-prediction needs a list without it (leading spacing), or use v-prediction", t);
  return TSD_OK;
}

int sampler_coeffs_ex(int kind, double eta, const std::vector<float>& ac, const std::vector<int>& ts, int i, int have_history,
                      int prediction, double out[8]) {
  TSD_TRY(sampler_prediction_ok(prediction, ac, ts));
  return prediction == TSD_PRED_V ? sampler_coeffs_v(kind, eta, ac, ts, i, have_history, out)
                                  : sampler_coeffs(kind, eta, ac, ts, i, have_history, out);
}

// scalar coefficients of `DDPMSampler.step` sampler.mojo:81-98 and `get_variance` :53-65 (fp32 like the reference).  `prev` is the
// reference's t - N // n (get_previous_timestep :46-51) under LEADING spacing and the next entry of the list under TRAILING.
static void ddpm_coeffs(const std::vector<float>& ac, int t, int prev, float* sa, float* sb, float* c_x0, float* c_xt, float* sigma) {
  const float a_t = ac[t];
  const float a_prev = prev >= 0 ? ac[prev] : 1.f;
  const float b_t = 1.f - a_t, b_prev = 1.f - a_prev;
  const float cur_a = a_t / a_prev, cur_b = 1.f - cur_a;
  *sa = sqrtf(a_t); *sb = sqrtf(b_t);
  *c_x0 = sqrtf(a_prev) * cur_b / b_t;
  *c_xt = sqrtf(cur_a) * b_prev / b_t;
  float var = b_prev / b_t * cur_b;
  if (var < 1e-20f) var = 1e-20f;
  *sigma = t > 0 ? sqrtf(var) : 0.f;
}

int sampler_step_plan(int kind, double eta, int spacing, int n_train, int n_infer, const std::vector<float>& ac,
                      const std::vector<int>& ts, int i, bool hist_valid, int prediction, SlotEntry* e) {
  if (i < 0 || i >= (int)ts.size()) TSD_FAIL(TSD_E_ARG, "sampler: step %d out of range (%d steps)", i, (int)ts.size());
  e->flags = 0;
  if (prediction == TSD_PRED_V) {
    // Every sampler, DDPM included, is an LMS entry from the v rows (double, rounded to float once here): the fp32 DDPM kernel restates a
    // reference that has no v-prediction.  Noise wherever c_n != 0; only DPM-Solver++(2M) reads or keeps the history.
    const bool multistep = kind == TSD_SAMPLER_DPMPP_2M, have_hist = multistep && hist_valid;
    double cd[8];
    TSD_TRY(sampler_coeffs_ex(kind, eta, ac, ts, i, have_hist ? 1 : 0, TSD_PRED_V, cd));
    e->mode = SLOT_LMS;
    for (int k = 0; k < 6; k++) e->c[k] = (float)cd[2 + k];
    if (have_hist) e->flags |= SLOT_HIST_IN;
    if (multistep) e->flags |= SLOT_HIST_OUT;
    if (e->c[5] != 0.f) e->flags |= SLOT_NOISE;
    return TSD_OK;
  }
  if (prediction != TSD_PRED_EPSILON) TSD_FAIL(TSD_E_ARG, "sampler: prediction type %d (0 epsilon, 1 v)", prediction);
  if (kind == TSD_SAMPLER_DDPM) {  // takes noise on every step that does not land on t = 0; no history
    const int t = ts[i];
    const int prev = spacing == TSD_SPACING_LEADING ? t - n_train / n_infer : (i + 1 < (int)ts.size() ? ts[i + 1] : -1);
    e->mode = SLOT_DDPM;
    ddpm_coeffs(ac, t, prev, &e->c[0], &e->c[1], &e->c[2], &e->c[3], &e->c[4]);
    e->c[5] = 0.f;
    if (t > 0) e->flags |= SLOT_NOISE;
    return TSD_OK;
  }
  // DDIM / DPM-Solver++(2M): the scalars of sampler_coeffs (double), rounded to float once here.  DPM-Solver++(2M) is the only one that
  // reads or keeps the history, and it takes no noise.
  const bool multistep = kind == TSD_SAMPLER_DPMPP_2M, have_hist = multistep && hist_valid;
  double cd[8];
  TSD_TRY(sampler_coeffs(kind, eta, ac, ts, i, have_hist ? 1 : 0, cd));
  e->mode = SLOT_LMS;
  for (int k = 0; k < 6; k++) e->c[k] = (float)cd[2 + k];
  if (have_hist) e->flags |= SLOT_HIST_IN;
  if (multistep) e->flags |= SLOT_HIST_OUT;
  if (!multistep && e->c[5] != 0.f) e->flags |= SLOT_NOISE;
  return TSD_OK;
}

extern "C" int tsd_sampler_timesteps(int spacing, int n_train, int n_infer, int start_step, int* timesteps, int cap) {
  std::vector<int> ts;
  TSD_TRY(sampler_timesteps(spacing, n_train, n_infer, start_step, ts));
  if (timesteps)
    for (int k = 0; k < (int)ts.size() && k < cap; k++) timesteps[k] = ts[k];
  return (int)ts.size();
}

extern "C" int tsd_sampler_alphas_cumprod(int n_train, int zero_terminal_snr, float* out, int cap) {
  if (n_train <= 0) TSD_FAIL(TSD_E_ARG, "schedule: train=%d", n_train);
  std::vector<float> ac;
  TSD_TRY(sampler_alphas_cumprod(n_train, zero_terminal_snr, ac));
  if (out)
    for (int k = 0; k < n_train && k < cap; k++) out[k] = ac[k];
  return n_train;
}

extern "C" int tsd_sampler_coeffs_ex(int kind, double eta, int spacing, int n_train, int n_infer, int start_step, int i,
                                     int have_history, int prediction, int zero_terminal_snr, double out[8]) {
  if (!out) TSD_FAIL(TSD_E_ARG, "tsd_sampler_coeffs_ex: argument 'out' is NULL");
  std::vector<int> ts;
  TSD_TRY(sampler_timesteps(spacing, n_train, n_infer, start_step, ts));
  std::vector<float> ac;
  TSD_TRY(sampler_alphas_cumprod(n_train, zero_terminal_snr, ac));
  return sampler_coeffs_ex(kind, eta, ac, ts, i, have_history, prediction, out);
}

extern "C" int tsd_sampler_coeffs(int kind, double eta, int spacing, int n_train, int n_infer, int start_step, int i,
                                  int have_history, double out[8]) {
  if (!out) TSD_FAIL(TSD_E_ARG, "tsd_sampler_coeffs: argument 'out' is NULL");
  return tsd_sampler_coeffs_ex(kind, eta, spacing, n_train, n_infer, start_step, i, have_history, TSD_PRED_EPSILON, 0, out);
}
