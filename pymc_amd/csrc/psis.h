// Pareto-smoothed importance sampling for leave-one-out (ArviZ's `psislw` / `_gpdfit` / `_gpinv` on the log scale; Vehtari, Simpson,
// Gelman, Yao, Gabry, "Pareto smoothed importance sampling"; the fit is Zhang & Stephens 2009), per observation, from a STREAMING
// state: the K1 = M + 1 smallest log-likelihood values of the observation (its M + 1 largest log importance ratios -ll) and one
// running log-sum (m_rest, r_rest) of -ll over every draw that is not among them.  A header the system C++ compiler and hipcc
// both accept: k_psis_fold / k_psis_finish (loglik_kernel.h) call it on the device, tests/psis_check.cpp wraps it in a stand-alone
// host program that tests/test_psis_host.py holds to the NumPy restatement (tests/psis_reference.py).
//
// With c = max(-ll) = -keep[0], t = -keep - c, xc = max(t[K1 - 1], log DBL_MIN), the tail the tl kept values with t > xc and sm
// their smoothed values (sm = t when nothing is smoothed):
//   elpd_loo_i = -c + log((S - tl) + sum_tail exp(sm - t)) - log(R + sum_{kept, not tail} exp(t) + sum_tail exp(sm)),
//   R = r_rest exp(m_rest - c).
// A value rejected by or evicted from the kept set is at most the (M + 1)-th largest ratio, so it is never in the tail: R is summed
// as values leave and nothing is ever subtracted from a total.
//
// psis_fit returns the same fit as a record (PsisFit) and psis_weight the normalised smoothed weight of one draw from it: what the
// second pass of LOO-PIT (loo_pit_kernel.h) weights the replicates of each draw with, held to tests/loo_pit_reference.py by
// tests/loo_pit_check.cpp / tests/test_loo_pit_host.py.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSIS_HD __host__ __device__ __forceinline__
#else
#define PSIS_HD inline
#endif

#define PSIS_K1_MAX 1024   // cap of K1 (about 116 000 draws at reff = 1)
#define PSIS_M_EST_MAX 61  // 30 + floor(sqrt(tail length)), tail length < PSIS_K1_MAX
#define PSIS_WORK (2 * PSIS_M_EST_MAX)   // doubles of work space psis_finish needs

// M = ceil(min(S / 5, 3 sqrt(S / reff)))
PSIS_HD int64_t psis_tail_len(int64_t S, double reff) {
  return (int64_t)ceil(fmin((double)S / 5.0, 3.0 * sqrt((double)S / reff)));
}

// One more term u = -ll of the running log-sum (m, r): r = sum exp(u - m), rescaled when the maximum moves (as k_waic_fold does).
// u = NaN or -inf (ll = NaN or +inf) poisons r with NaN for good.  u = +inf (ll = -inf: psis_finish answers from keep[0] alone)
// only marks m, so that neither inf - inf nor 0 * inf is ever formed and an earlier NaN stays.
PSIS_HD void psis_rest_fold(double u, double& m, double& r) {
  if (u == INFINITY) m = u;
  else if (u > m) { r = (m == -INFINITY ? r : r * exp(m - u)) + 1.0; m = u; }
  else if (u > -INFINITY) r += exp(u - m);
  else r = NAN;
}

// Insert v (below keep[K1 - 1], the caller has compared) into the ascending column keep[j * stride], j < K1, shifting from the bottom;
// returns the value that fell off (+inf: an empty slot).  On the device the lanes of a wave walk j together.  The rows above the
// free slot are read PSIS_CHUNK at a time before any of them is compared: the walk is a chain of dependent reads otherwise (the
// exit test needs the value), and its latency, not its bytes, is what an insert costs.
#define PSIS_CHUNK 8
PSIS_HD double psis_insert(double* keep, int64_t stride, int K1, double v) {
  const double out = keep[(int64_t)(K1 - 1) * stride];
  int j = K1 - 1;   // the free slot
  bool placed = false;
  while (j > 0 && !placed) {
    const int j0 = j;
    double p[PSIS_CHUNK];
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int u = 0; u < PSIS_CHUNK; ++u) p[u] = u < j0 ? keep[(int64_t)(j0 - 1 - u) * stride] : 0.0;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int u = 0; u < PSIS_CHUNK; ++u) {
      if (u < j0 && !placed) {
        if (p[u] > v) { keep[(int64_t)(j0 - u) * stride] = p[u]; j = j0 - u - 1; }
        else placed = true;
      }
    }
  }
  keep[(int64_t)j * stride] = v;
  return out;
}

// gpinv(p, k, s): the quantile of the generalised Pareto distribution; NaN when s <= 0
PSIS_HD double psis_gpinv(double p, double k, double s) {
  if (!(s > 0.0)) return NAN;
  if (fabs(k) < DBL_EPSILON) return -s * log1p(-p);
  return s * expm1(-k * log1p(-p)) / k;
}

struct PsisOut { double khat, elpd; };

// The fit of one observation as a record: everything the smoothed weight of ANY of its draws follows from (psis_weight), so that a
// second pass over the draws can weight them one by one.  logden = log(R + sum_{kept, not tail} exp t + sum_tail exp sm), the
// normaliser of the identity above.
#define PSIS_FIT_OK 0
#define PSIS_FIT_DEGENERATE 1   // keep[0] = -inf: the left-out density is 0, elpd = -inf
#define PSIS_FIT_POISONED 2     // r_rest NaN: a NaN or +inf value
#define PSIS_FIT_FIELDS 7       // c, xc, tl, khat, sigma, logden, state (the order of a [PSIS_FIT_FIELDS][N] block)
struct PsisFit { double c, xc, khat, sigma, logden; int tl, state; };

// keep: the column of K1 = psis_tail_len(S, reff) + 1 values after all S draws (reff enters through K1 alone; the caller passes the
// K1 the column was allocated with); work[j * wstride], j < PSIS_WORK: the fit's candidates (registers, LDS or the stack).
// num = sum_tail exp(sm - t), the one term of elpd_loo_i that is not part of the record.
PSIS_HD PsisFit psis_fit_num(const double* keep, int64_t stride, int K1, double m_rest, double r_rest, double* work, int wstride, double& num_out) {
  PsisFit f;
  f.c = NAN; f.xc = NAN; f.khat = NAN; f.sigma = NAN; f.logden = NAN; f.tl = 0; f.state = PSIS_FIT_OK;
  num_out = NAN;
  if (r_rest != r_rest) { f.state = PSIS_FIT_POISONED; return f; }                          // a NaN or +inf value
  const double k0 = keep[0];
  if (k0 == -INFINITY) { f.khat = INFINITY; f.state = PSIS_FIT_DEGENERATE; return f; }      // the left-out density is 0
  const double c = -k0;
#define PSIS_T(j) (-keep[(int64_t)(j) * stride] - c)
  const double xc = fmax(PSIS_T(K1 - 1), log(DBL_MIN)), exc = exp(xc);
  int tl = 0;
  while (tl < K1 && PSIS_T(tl) > xc) ++tl;   // (t descends along the column)
  double khat = INFINITY, sigma = 0.0;
  if (tl > 4) {
    // a ascending = the tail read from its end: a[jj] = exp(t[tl - 1 - jj]) - exp(xc)
    const int n = tl, m_est = 30 + (int)floor(sqrt((double)n));
    const double aq = exp(PSIS_T(tl - 1 - ((int)floor((double)n / 4.0 + 0.5) - 1))) - exc, amax = exp(PSIS_T(0)) - exc;
    double* wb = work;                                   // b_j
    double* wk = work + (int64_t)PSIS_M_EST_MAX * wstride;   // sum log1p(-b_j a), then L_j
    for (int j = 0; j < m_est; ++j) {
      wb[(int64_t)j * wstride] = (1.0 - sqrt((double)m_est / ((double)(j + 1) - 0.5))) / (3.0 * aq) + 1.0 / amax;
      wk[(int64_t)j * wstride] = 0.0;
    }
    for (int jj = 0; jj < n; ++jj) {   // one read of the tail for all candidates
      const double a = exp(PSIS_T(tl - 1 - jj)) - exc;
      for (int j = 0; j < m_est; ++j) wk[(int64_t)j * wstride] += log1p(-wb[(int64_t)j * wstride] * a);
    }
    for (int j = 0; j < m_est; ++j) {
      const double kj = wk[(int64_t)j * wstride] / (double)n;
      wk[(int64_t)j * wstride] = (double)n * (log(-(wb[(int64_t)j * wstride] / kj)) - kj - 1.0);
    }
    double sw = 0.0, sbw = 0.0;
    for (int j = 0; j < m_est; ++j) {
      const double Lj = wk[(int64_t)j * wstride];
      double s = 0.0;
      for (int i = 0; i < m_est; ++i) s += exp(wk[(int64_t)i * wstride] - Lj);
      const double w = 1.0 / s;
      if (w >= 10.0 * DBL_EPSILON) { sw += w; sbw += wb[(int64_t)j * wstride] * w; }
    }
    const double b = sbw / sw;
    double ks = 0.0;
    for (int jj = 0; jj < n; ++jj) ks += log1p(-b * (exp(PSIS_T(tl - 1 - jj)) - exc));
    const double k = ks / (double)n;
    sigma = -k / b;
    khat = ((double)n * k + 5.0) / ((double)n + 10.0);
  }
  const bool smooth = khat - khat == 0.0;   // finite
  double num = 0.0, den_tail = 0.0, den_kept = 0.0;
  for (int j = 0; j < K1; ++j) {
    const double t = PSIS_T(j);
    if (j < tl) {
      double sm = t;
      if (smooth) {   // (a NaN quantile, sigma <= 0, stays NaN)
        sm = log(psis_gpinv(((double)(tl - 1 - j) + 0.5) / (double)tl, khat, sigma) + exc);
        if (sm > 0.0) sm = 0.0;
      }
      num += exp(sm - t);
      den_tail += exp(sm);
    } else
      den_kept += exp(t);
  }
#undef PSIS_T
  const double R = m_rest == -INFINITY ? 0.0 : r_rest * exp(m_rest - c);
  f.c = c; f.xc = xc; f.tl = tl; f.khat = khat; f.sigma = sigma;
  f.logden = log(R + den_kept + den_tail);
  num_out = num;
  return f;
}

PSIS_HD PsisFit psis_fit(const double* keep, int64_t stride, int K1, double m_rest, double r_rest, int64_t S, double* work, int wstride) {
  (void)S;   // (the record does not depend on it: S enters elpd_loo_i alone)
  double num;
  return psis_fit_num(keep, stride, K1, m_rest, r_rest, work, wstride, num);
}

PSIS_HD PsisOut psis_finish(const double* keep, int64_t stride, int K1, double m_rest, double r_rest, int64_t S, double* work, int wstride) {
  PsisOut o;
  double num;
  const PsisFit f = psis_fit_num(keep, stride, K1, m_rest, r_rest, work, wstride, num);
  if (f.state == PSIS_FIT_POISONED) { o.khat = NAN; o.elpd = NAN; return o; }
  if (f.state == PSIS_FIT_DEGENERATE) { o.khat = INFINITY; o.elpd = -INFINITY; return o; }
  o.khat = f.khat;
  o.elpd = -f.c + log((double)(S - f.tl) + num) - f.logden;
  return o;
}

// The smoothed value of rank j < tl of the tail, exactly as psis_fit_num forms it; t_j = -keep[j] - c.
PSIS_HD double psis_smoothed(const PsisFit& f, double t_j, int j) {
  if (!(f.khat - f.khat == 0.0)) return t_j;   // nothing is smoothed
  double sm = log(psis_gpinv(((double)(f.tl - 1 - j) + 0.5) / (double)f.tl, f.khat, f.sigma) + exp(f.xc));
  if (sm > 0.0) sm = 0.0;
  return sm;
}

// The normalised Pareto-smoothed weight of a draw whose log-likelihood is v, from the record and the sorted column: the weights of
// all S draws of the first pass sum to 1.  A draw outside the tail (t = -v - c <= xc) keeps its raw weight exp(t - logden).  A draw
// of the tail takes the smoothed value of its RANK, which is its position in keep[0 .. tl).
//
// Ties.  ArviZ hands tied ratios different smoothed weights in the order the draws happen to be stored (a stable argsort), so its
// result depends on the order of the trace.  Here a value that occupies the ranks [j0, j1) takes the ARITHMETIC MEAN of their
// weights: the sum of the weights stays 1, the result does not depend on the order of the draws, and it is ArviZ's whenever a
// value occurs once.  A v that is not in the column (the caller streamed draws the first pass did not see) takes the weight of its
// insertion rank; the weights then no longer sum to 1, which is how the misuse is noticed.
PSIS_HD double psis_weight(const PsisFit& f, const double* keep, int64_t stride, double v) {
  if (f.state != PSIS_FIT_OK) return NAN;
  const double t = -v - f.c;
  if (!(t > f.xc) || f.tl == 0) return exp(t - f.logden);   // (a NaN value stays NaN; an empty tail has no rank to give)
  int j0 = 0, n = f.tl;                        // lower bound: the first rank whose value is not below v
  while (n > 0) {
    const int h = n >> 1;
    if (keep[(int64_t)(j0 + h) * stride] < v) { j0 += h + 1; n -= h + 1; } else n = h;
  }
  int j1 = j0;
  while (j1 < f.tl && keep[(int64_t)j1 * stride] == v) ++j1;
  if (j1 == j0) {                              // not found: the insertion rank
    if (j0 >= f.tl) j0 = f.tl - 1;
    j1 = j0 + 1;
  }
  double s = 0.0;
  for (int j = j0; j < j1; ++j) s += exp(psis_smoothed(f, -keep[(int64_t)j * stride] - f.c, j) - f.logden);
  return j1 - j0 == 1 ? s : s / (double)(j1 - j0);
}
