// The scalar pieces of the convergence summary of a trace (`az.summary(kind="all")`; Vehtari, Gelman, Simpson, Carpenter, Buerkner
// 2021, "Rank-normalization, folding, and localization"; pymc_amd/stats.py states two of the estimators for the host): the inverse
// normal CDF, the Geyer scan behind every ESS, the HDI scan, NumPy's linear quantile and the R-hat formula.  A header the system
// C++ compiler and hipcc both accept: k_summary (summary_kernel.h) calls it on the device, tests/summary_check.cpp wraps it in a
// stand-alone host program that tests/test_summary_host.py holds to the NumPy restatement (tests/summary_reference.py).
//
// Nothing here sums over draws: the autocovariances reach the Geyer scan through a callable, "the mean over chains of the
// autocovariance at lag t", which the caller evaluates however it likes and only for the lags the scan asks for -- a mixing chain
// stops it after a few.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SM_HD __host__ __device__ __forceinline__
#else
#define SM_HD inline
#endif
// NumPy rounds every product and sum of the quantile's index and interpolation on its own; the device compiler would contract them
// into fused multiply-adds (host builds of this header use -ffp-contract=off)
#if defined(__HIP_DEVICE_COMPILE__)
#define SM_MUL(a, b) __dmul_rn((a), (b))
#define SM_ADD(a, b) __dadd_rn((a), (b))
#else
#define SM_MUL(a, b) ((a) * (b))
#define SM_ADD(a, b) ((a) + (b))
#endif

#define SM_COLS 9
enum { SM_MEAN = 0, SM_SD = 1, SM_HDI_LO = 2, SM_HDI_HI = 3, SM_MCSE_MEAN = 4, SM_MCSE_SD = 5, SM_ESS_BULK = 6, SM_ESS_TAIL = 7, SM_R_HAT = 8 };

// Python's max(a, b) / min(a, b): the first argument unless the second compares beyond it (a NaN first argument stays)
SM_HD double sm_pymax(double a, double b) { return b > a ? b : a; }
SM_HD double sm_pymin(double a, double b) { return b < a ? b : a; }

// ---- the inverse normal CDF: Wichura, "Algorithm AS 241: The percentage points of the normal distribution", PPND16 ---------------
// 0 < p < 1 (0 and 1 give -inf and +inf).  Three rational approximations: |p - 1/2| <= 0.425, and in r = sqrt(-log(min(p, 1 - p)))
// on either side of r = 5.
SM_HD double sm_ndtri(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    return q * (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                    1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) /
           (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
               5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0);
  }
  double r = q < 0.0 ? p : 1.0 - p;
  if (!(r > 0.0)) return r == 0.0 ? (q < 0.0 ? -INFINITY : INFINITY) : NAN;
  r = sqrt(-log(r));
  double v;
  if (r <= 5.0) {
    r -= 1.6;
    v = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
            3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0) /
        (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
            6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r + 2.05319162663775882187e+0) * r + 1.0);
  } else {
    r -= 5.0;
    v = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
            2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0) /
        (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
            1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0);
  }
  return q < 0.0 ? -v : v;
}

// the z-score of an average rank r (1-based) among `size` values
SM_HD double sm_rank_z(double r, int64_t size) { return sm_ndtri((r - 0.375) / ((double)size + 0.25)); }

// ---- ESS of c chains of n draws: stats._ess_raw -----------------------------------------------------------------------------------
// acov0 = the mean over chains of the biased autocovariance at lag 0, var_means = the variance (ddof = 1) of the chain means (unused
// when c == 1), acov_at(t) = the same mean at lag t, 1 <= t < n, asked for in increasing t.  The reference fills an array rho[] and
// then makes its pair sums monotone and adds them; here a pair is made monotone and added when the next one is asked for, so nothing
// is stored: a pair enters the sum only if the scan went on past it, and the pair the scan stopped at contributes its first value
// alone (when that is positive, or when the pair's sum is not negative).
template <class AcovAt>
SM_HD double sm_ess(int64_t c, int64_t n, double acov0, double var_means, AcovAt&& acov_at) {
  if (n < 4) return NAN;
  const double mean_var = acov0 * (double)n / ((double)n - 1.0);
  double var_plus = mean_var * ((double)n - 1.0) / (double)n;
  if (c > 1) var_plus += var_means;
  if (var_plus == 0.0) return (double)(c * n);
  double even = 1.0, odd = 1.0 - (mean_var - acov_at((int64_t)1)) / var_plus;
  double sum = 0.0, pa = 0.0, pb = 0.0;
  bool first = true, stored = true;
  int64_t t = 1;
  while (t < n - 3 && even + odd > 0.0) {
    if (!first && even + odd > pa + pb) { even = (pa + pb) / 2.0; odd = even; }
    sum += even; sum += odd;
    pa = even; pb = odd; first = false;
    even = 1.0 - (mean_var - acov_at(t + 1)) / var_plus;
    odd = 1.0 - (mean_var - acov_at(t + 2)) / var_plus;
    stored = even + odd >= 0.0;
    t += 2;
  }
  double tail;
  if (first) { sum = 1.0; tail = 1.0; }   // no pair beyond (rho_0, rho_1): rho[max_t + 1] = rho_even = 1
  else tail = even > 0.0 ? even : (stored ? even : 0.0);
  const double tau = -1.0 + 2.0 * sum + tail;
  return (double)(c * n) / sm_pymax(tau, 1.0 / log10((double)(c * n)));
}

// ---- split R-hat of one array of c chains of n draws -----------------------------------------------------------------------------
// W = the mean over chains of the chain variances (ddof = 1), B = n times the variance (ddof = 1) of the chain means
SM_HD double sm_rhat(int64_t n, double W, double B) {
  return sqrt(((double)(n - 1) / (double)n * W + B / (double)n) / W);
}

// ---- HDI -------------------------------------------------------------------------------------------------------------------------
SM_HD int64_t sm_hdi_k(double hdi_prob, int64_t S) { return (int64_t)floor(hdi_prob * (double)S); }
// The narrowest xs[i + k] - xs[i] over i = start, start + stride, ... < S - k, the first such i on ties; best_w = +inf, best_i = -1
// when the range is empty.  (width, i) pairs of several ranges combine through sm_hdi_better.
SM_HD void sm_hdi_scan(const double* xs, int64_t S, int64_t k, int64_t start, int64_t stride, double& best_w, int64_t& best_i) {
  best_w = INFINITY; best_i = -1;
  for (int64_t i = start; i < S - k; i += stride) {
    const double w = xs[i + k] - xs[i];
    if (best_i < 0 || w < best_w) { best_w = w; best_i = i; }
  }
}
SM_HD bool sm_hdi_better(double w, int64_t i, double best_w, int64_t best_i) {
  return i >= 0 && (best_i < 0 || w < best_w || (w == best_w && i < best_i));
}

// ---- numpy.quantile(xs, q), method "linear", of n sorted finite values -------------------------------------------------------------
// the method's virtual index (n - 1) q, _get_indexes, _get_gamma and _lerp of numpy/lib/_function_base_impl.py, operation by operation
SM_HD double sm_quantile(const double* xs, int64_t n, double q) {
  const double vi = SM_MUL((double)(n - 1), q);
  if (vi >= (double)(n - 1)) return xs[n - 1];
  if (vi < 0.0) return xs[0];
  const double prev = floor(vi), t = SM_ADD(vi, -prev);
  const double a = xs[(int64_t)prev], b = xs[(int64_t)prev + 1];
  const double diff = SM_ADD(b, -a);
  return t >= 0.5 ? SM_ADD(b, -SM_MUL(diff, SM_ADD(1.0, -t))) : SM_ADD(a, SM_MUL(diff, t));
}

// ---- the columns that are arithmetic on sums ---------------------------------------------------------------------------------------
// d = (x - mean)^2 over all S draws: sum_d = sum d, sum_d2 = sum d^2
SM_HD double sm_sd(double sum_d, int64_t S) { return sqrt(sum_d / (double)(S - 1)); }
SM_HD double sm_mcse_sd(double sum_d, double sum_d2, int64_t S, double ess_d) {
  const double ev = sum_d / (double)S;
  return sqrt((sum_d2 / (double)S - ev * ev) / ess_d / ev / 4.0);
}
