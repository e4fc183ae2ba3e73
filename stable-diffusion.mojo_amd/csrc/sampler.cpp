// sampler.cpp - host side of the denoise schedule: the alphas_cumprod table, the timestep lists and the per-step scalars of the
// samplers (no GPU).  The table is the reference's fp32 Tensor (sampler.mojo:28-32); everything derived from it here is computed in
// double and rounded to float once, where the kernel takes it (kernels_sampler.hip).  The session's DDPM path does not come through
// sampler_coeffs: it keeps the reference's fp32 scalars (ddpm_coeffs below) and its own kernel.  sampler_step_plan is the one place
// that turns a schedule index into what an update launch is given, for the lockstep step and for a slot alike (session.cpp).
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
                      const std::vector<int>& ts, int i, bool hist_valid, SlotEntry* e) {
  if (i < 0 || i >= (int)ts.size()) TSD_FAIL(TSD_E_ARG, "sampler: step %d out of range (%d steps)", i, (int)ts.size());
  e->flags = 0;
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

extern "C" int tsd_sampler_coeffs(int kind, double eta, int spacing, int n_train, int n_infer, int start_step, int i,
                                  int have_history, double out[8]) {
  if (!out) TSD_FAIL(TSD_E_ARG, "tsd_sampler_coeffs: argument 'out' is NULL");
  std::vector<int> ts;
  TSD_TRY(sampler_timesteps(spacing, n_train, n_infer, start_step, ts));
  std::vector<float> ac;
  sampler_alphas_cumprod(n_train, ac);
  return sampler_coeffs(kind, eta, ac, ts, i, have_history, out);
}
