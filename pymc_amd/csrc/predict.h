// Predictions at new data: the conditional mean and variance of one observation given its factor's arguments, and the fold that
// turns the per-draw values of an observation into its posterior-predictive summary (include/nuts_mi355.h, nuts_model_predict_moments
// / nuts_pred_*).  A header the system C++ compiler and hipcc both accept: k_pd_fold_* / k_pd_moments_* (predict_kernel.h) call it
// on the device, tests/predict_check.cpp wraps it in a stand-alone host program that tests/test_predict_host.py holds to the NumPy
// restatement (tests/predict_reference.py).
//
// Argument conventions: those of pp_draw (predictive.h) and dist_eval_body (model_dev.h) -- (a1, a2, a3) are the factor's arguments
// 1 .. 3, argument 0 (the observed value) is not read.
//
//   family            a1, a2, a3          mean                         variance
//   Normal            mu, sigma           mu                           sigma^2
//   HalfNormal        sigma               sigma sqrt(2 / pi)           sigma^2 (1 - 2 / pi)
//   Cauchy            alpha, beta         NaN                          NaN
//   HalfCauchy        beta                +inf                         NaN
//   StudentT          nu, mu, sigma       nu <= 1: NaN; else mu        nu <= 1: NaN; nu <= 2: +inf; else sigma^2 nu / (nu - 2)
//   Beta              alpha, beta         alpha / (alpha + beta)       alpha beta / ((alpha + beta)^2 (alpha + beta + 1))
//   Exponential       lam                 1 / lam                      1 / lam^2
//   Uniform           lower, upper        (lower + upper) / 2          (upper - lower)^2 / 12
//   Bernoulli-logit   eta                 p = sigmoid_d(eta)           sigmoid_d(eta) sigmoid_d(-eta)  (no cancellation for large |eta|)
//   LogNormal         mu, sigma           exp(mu + sigma^2 / 2)        expm1(sigma^2) exp(2 mu + sigma^2)
//   Bernoulli         p                   p                            p (1 - p)
//   Binomial          n, p                n p                          n p (1 - p)
//   Gamma             alpha, beta         alpha / beta                 alpha / beta^2
//   InverseGamma      alpha, beta         alpha <= 1: +inf; else       alpha <= 1: NaN; alpha <= 2: +inf; else
//                                         beta / (alpha - 1)           beta^2 / ((alpha - 1)^2 (alpha - 2))
//   Laplace           mu, b               mu                           2 b^2
//   Poisson           mu                  mu                           mu
// A moment that diverges is +inf, one that does not exist is NaN.  Invalid parameters -- the conditions of KILL_PARAM in
// dist_eval_body, as pp_draw restates them -- give NaN for both.  TruncatedNormal, Potential and derived vectors are refused
// (pd_family_ok).
#pragma once
#include <math.h>
#include <stdint.h>

#include "predictive.h"

#define PD_ACC_ROWS 6   // accumulator rows per observation: mean and M2 of m, mean of v, (max, sum) of lp, count

// the families pd_moments covers: what pp_draw draws from, and Binomial
PP_HD bool pd_family_ok(int dist) { return pp_family_ok(dist) || dist == PP_D_BINOMIAL; }

PP_HD void pd_moments(int dist, double konst, double a1, double a2, double a3, double* mean, double* var) {
  (void)konst;
  double m = NAN, v = NAN;
  switch (dist) {
    case PP_D_NORMAL: if (a2 > 0) { m = a1; v = a2 * a2; } break;
    case PP_D_HALFNORMAL: if (a1 > 0) { m = a1 * 0.79788456080286535588; v = a1 * a1 * 0.36338022763241865692; } break;
    case PP_D_CAUCHY: break;
    case PP_D_HALFCAUCHY: if (a1 > 0) m = INFINITY; break;
    case PP_D_STUDENTT:
      if (a1 > 0 && a3 > 0 && a1 > 1.0) { m = a2; v = a1 > 2.0 ? a3 * a3 * (a1 / (a1 - 2.0)) : INFINITY; }
      break;
    case PP_D_BETA:
      if (a1 > 0 && a2 > 0) { const double s = a1 + a2; m = a1 / s; v = a1 * a2 / (s * s * (s + 1.0)); }
      break;
    case PP_D_EXPONENTIAL: if (a1 > 0) { m = 1.0 / a1; v = m * m; } break;
    case PP_D_UNIFORM: if (a1 <= a2) { const double w = a2 - a1; m = 0.5 * (a1 + a2); v = w * w / 12.0; } break;
    case PP_D_BERNOULLI_LOGIT: if (a1 == a1) { m = sigmoid_d(a1); v = m * sigmoid_d(-a1); } break;
    case PP_D_LOGNORMAL:
      if (a2 > 0) { const double s2 = a2 * a2; m = exp(a1 + 0.5 * s2); v = expm1(s2) * exp(2.0 * a1 + s2); }
      break;
    case PP_D_BERNOULLI: if (a1 >= 0 && a1 <= 1) { m = a1; v = a1 * (1.0 - a1); } break;
    case PP_D_BINOMIAL: if (a1 >= 0 && a2 >= 0 && a2 <= 1) { m = a1 * a2; v = m * (1.0 - a2); } break;
    case PP_D_GAMMA: {
      const double be = 1.0 / (1.0 / a2);   // (as the density takes it)
      if (a1 > 0 && be > 0) { m = a1 / be; v = m / be; }
    } break;
    case PP_D_INVGAMMA:
      if (a1 > 0 && a2 > 0) {
        if (a1 > 1.0) {
          m = a2 / (a1 - 1.0);
          v = a1 > 2.0 ? m * m / (a1 - 2.0) : INFINITY;
        } else m = INFINITY;
      }
      break;
    case PP_D_LAPLACE: if (a2 > 0) { m = a1; v = 2.0 * a2 * a2; } break;
    case PP_D_POISSON: if (a1 >= 0) { m = a1; v = a1; } break;
    default: break;
  }
  *mean = m; *var = v;
}

// marginal Normal mixture, w[k] the weights: mean = sum w_k mu_k, var = sum w_k (sigma_k^2 + (mu_k - mean)^2), both in index order
PP_HD void pd_mixture(int K, const double* mu, const double* sigma, const double* w, double* mean, double* var) {
  double m = 0.0, v = 0.0;
  for (int k = 0; k < K; ++k) m += w[k] * mu[k];
  for (int k = 0; k < K; ++k) { const double d = mu[k] - m; v += w[k] * (sigma[k] * sigma[k] + d * d); }
  *mean = m; *var = v;
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------
// One observation's state over the draws folded so far: Welford's mean and M2 of the conditional mean m, the running mean of the
// conditional variance v, the running log-sum-exp of lp as (max, sum relative to the max) -- k_waic_fold's recurrence -- and the
// count.  NaN is not hidden: an observation that met a NaN moment stays NaN.  An infinite moment makes the running mean infinite
// (what the sum of the values would be), never NaN by inf - inf.  lp = -inf carries weight 0 and never forms -inf - -inf.
struct PDAcc { double mean, M2, vbar, lmax, lsum, count; };

PP_HD PDAcc pd_acc_init() { return PDAcc{0.0, 0.0, 0.0, -INFINITY, 0.0, 0.0}; }

// mean of k values from the mean of the first k - 1 and the k-th, x
PP_HD double pd_run_mean(double mean, double x, double k) {
  if (x != x || mean != mean) return NAN;
  const bool xi = x == INFINITY || x == -INFINITY, mi = mean == INFINITY || mean == -INFINITY;
  if (xi && mi) return x == mean ? mean : NAN;
  if (mi) return mean;
  if (xi) return x;
  return mean + (x - mean) / k;
}

PP_HD void pd_fold(PDAcc* a, double m, double v, double lp, bool with_lp) {
  a->count += 1.0;
  const double dl = m - a->mean;
  a->mean = pd_run_mean(a->mean, m, a->count);
  a->M2 = a->M2 + dl * (m - a->mean);
  a->vbar = pd_run_mean(a->vbar, v, a->count);
  if (with_lp) {
    if (lp > a->lmax) { a->lsum = (a->lmax == -INFINITY ? 0.0 : a->lsum * exp(a->lmax - lp)) + 1.0; a->lmax = lp; }
    else if (lp > -INFINITY) a->lsum += lp == a->lmax ? 1.0 : exp(lp - a->lmax);
    else if (lp != lp) a->lsum = lp;   // (a NaN value is not hidden)
  }
}

// lpd = log mean_s exp(lp_s); -inf when every lp was
PP_HD double pd_lpd(const PDAcc* a) { return log(a->lsum) + a->lmax - log(a->count); }
