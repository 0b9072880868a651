// Power-scaling sensitivity (Kallioinen, Paananen, Buerkner, Vehtari 2023, "Detecting and diagnosing prior and likelihood sensitivity
// with power-scaling"; `az.psens`, the `priorsense` table): how far the posterior of one parameter moves when one component of the
// model -- the prior or the likelihood -- is raised to a power alpha next to 1.  A header the system C++ compiler and hipcc both
// accept: k_psens_weights / k_psens (psens_kernel.h) call it on the device, tests/psens_check.cpp wraps it in a stand-alone host
// program that tests/test_psens_host.py holds to the NumPy restatement (tests/psens_reference.py).  DESIGN.md 4.23.
//
// Weights.  lc[s] is the component's log-density at draw s; for alpha the raw log-ratio is (alpha - 1) lc[s].  v[s] = (1 - alpha) lc[s]
// (ps_column) is treated as the log-likelihood column of ONE observation in the sense of psis.h: tail length psis_tail_len(S, 1),
// psis_fit, psis_weight (tied values share the mean weight of their ranks), then divided by their sum (ps_normalise).  A tail of 4
// values or fewer is not smoothed (khat = +inf, the normalised raw ratios).  A non-finite lc makes every weight NaN.
//
// Distance.  x sorted ascending (ties by draw number), w permuted along; for j = 0 .. S - 2
//   bw_j = x_{j+1} - x_j,  P_j = (j + 1) / S,  Q_j = sum_{i <= j} w_i,  L(t) = log2 t (0 at t = 0),
//   Pi = sum bw P,  Qi = sum bw Q,  A = sum bw P (L(P) - L((P + Q) / 2)),  B = sum bw Q (L(Q) - L((P + Q) / 2))       (ps_term)
//   pq = max(A + (Qi - Pi) / (2 ln 2), 0),  qp = max(B + (Pi - Qi) / (2 ln 2), 0),  D = (pq + qp) / (Pi + Qi)          (ps_distance)
// cjs = sqrt D; the distance of -x is the same sums over the same sorted data walked from the top (bw_{S-2-j}, Q = total - Q_{S-2-j}).
//   cjs_lo = max(cjs(x, w_lo), cjs(-x, w_lo)), cjs_hi likewise, sensitivity = (cjs_lo + cjs_hi) / (2 log2(1 + delta))  (ps_sensitivity)
// A constant parameter (Pi + Qi = 0) gives NaN.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PS_HD __host__ __device__ __forceinline__
#else
#define PS_HD inline
#endif

#define PS_COLS 3          // cjs_lo cjs_hi sensitivity (NUTS_PSENS_COLS)
#define PS_CJS_LO 0
#define PS_CJS_HI 1
#define PS_SENS 2
#define PS_SUMS 4          // Pi, Qi, A, B
#define PS_INV_2LN2 0.72134752044448170368   // 1 / (2 ln 2)

// neither NaN nor +-inf.  (Not `v - v == 0`: where v is a product the device compiler contracts v - v into fma(a, b, -v), the
// product's rounding error, which is not 0.)
PS_HD bool ps_finite(double v) { return fabs(v) <= DBL_MAX; }

// the "log-likelihood column" psis.h is fed with: minus the raw log-ratio
PS_HD double ps_column(double alpha, double lc) { return (1.0 - alpha) * lc; }

// a weight over the sum of all S of them
PS_HD double ps_normalise(double w, double total) { return w / total; }

PS_HD double ps_log2(double t) { return t != 0.0 ? log2(t) : 0.0; }

// below 0 -> 0; a NaN stays
PS_HD double ps_clamp(double v) { return v < 0.0 ? 0.0 : v; }

// one element's terms of the four sums, added to acc[PS_SUMS]
PS_HD void ps_term(double bw, double P, double Q, double* acc) {
  const double lm = ps_log2((P + Q) / 2.0);
  acc[0] += bw * P;
  acc[1] += bw * Q;
  acc[2] += bw * P * (ps_log2(P) - lm);
  acc[3] += bw * Q * (ps_log2(Q) - lm);
}

// D from the four sums
PS_HD double ps_distance(const double* sums) {
  const double Pi = sums[0], Qi = sums[1];
  if (Pi + Qi == 0.0) return NAN;   // a constant parameter
  const double pq = ps_clamp(sums[2] + (Qi - Pi) * PS_INV_2LN2);
  const double qp = ps_clamp(sums[3] + (Pi - Qi) * PS_INV_2LN2);
  return (pq + qp) / (Pi + Qi);
}

// cjs of one alpha from the distance of x and of -x: the larger (NaN if either is)
PS_HD double ps_cjs(double d_fwd, double d_rev) {
  const double a = sqrt(d_fwd), b = sqrt(d_rev);
  if (a != a || b != b) return NAN;
  return a > b ? a : b;
}

PS_HD double ps_sensitivity(double cjs_lo, double cjs_hi, double delta) { return (cjs_lo + cjs_hi) / (2.0 * log2(1.0 + delta)); }
