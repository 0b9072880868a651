// Model comparison (`az.compare` on the log scale): the arithmetic of one observation and the stacking solver, in a
// header the system C++ compiler and hipcc both accept.  k_cmp_terms / k_cmp_stack_pass / k_cmp_bb (compare_kernel.h) call the
// per-observation part on the device, nuts_compare_stacking (engine.hip) runs the solver over the device's passes, and
// tests/compare_check.cpp wraps both in a stand-alone host program that tests/test_compare_host.py holds to the NumPy restatement
// (tests/compare_reference.py).
//
// e_ik: the pointwise elpd (LOO or WAIC) of observation i < N under model k < K, K <= CMP_MAXK.
//
// Bayesian bootstrap (BB-pseudo-BMA; Yao, Vehtari, Simpson, Gelman 2018, section 3.4).  Replicate b weighs the observations by a
// Dirichlet(1, ..., 1) vector alpha_b. = g(b, .) / sum_j g(b, j), g an Exp(1) variate.  The [b_samples][N] matrix never exists: g(b, i)
// is a function of (seed, b, i), recomputed where it is used, from the Philox block (predictive.h)
//   key = pp_key(seed),  counter = (i low 32, i high 32, b >> 1, CMP_TAG),  CMP_TAG = 0xFFFF0000  (kind 3, index 0x3fff, t = 0)
//   g(b, i) = -log(u),  u = u0 of the block for even b, u1 for odd b
// -- one block serves the replicates 2 j and 2 j + 1.  A GLM node (kind 3) always has index 0, so no posterior-predictive stream
// shares a counter with this one.  u is never 0 (predictive.h), so g is finite; u = 1 (probability 2^-53) gives g = 0.
//   z_bk = N (sum_i g(b, i) e_ik) / (sum_i g(b, i))
//
// Stacking (Yao et al. 2018, section 3.1): maximise f(w) = sum_i log sum_k w_k exp(e_ik) over the simplex.  Per observation
//   m_i = max_k e_ik,  p_ik = exp(e_ik - m_i),  f(w) = sum_i [m_i + log d_i],  d_i = sum_k w_k p_ik
// -- the shift changes neither the maximiser nor the gradient, and at least one p_ik is 1 where the unshifted exp(e_ik) is 0 for
// e_ik below -745.  With q_ik = p_ik / d_i a pass over the observations gives
//   sum_i log d_i,   g_k = (1 / N) sum_i q_ik,   H_kl = -(1 / N) sum_i q_ik q_il
// (gradient and Hessian of f / N).  sum_k w_k g_k = 1 at every w, so at the maximiser g_k <= 1 with equality where w_k > 0:
//   kkt_gap = max_k g_k - 1 >= 0,   f* - f(w) <= N kkt_gap   (concavity: f* - f(w) <= N g . (w* - w) <= N (max_k g_k - 1)).
//
// Solver (cmp_solve).  Start at w = 1 / K.  Each round: (1) the free face is {k: w_k > 0 or g_k > 1}; the others stay at 0.  (2) The
// Newton step on it solves [H 1; 1' 0] (delta, lambda) = (-g, 0) in the minimum-norm sense: the symmetric system is diagonalised
// (Jacobi) and eigen-directions below CMP_EIG_CUT of the largest |eigenvalue| are dropped -- duplicated models make H singular.  A
// freed weight at 0 whose step points outward is pinned again and the system solved anew.  (3) The step is capped where the first
// weight reaches 0 (that weight becomes exactly 0).  (4) It is halved, up to CMP_HALVINGS trials, while f falls by more than the
// rounding of its sum, 1e-13 max(1, |sum_i log d_i|).  (5) If no trial is accepted, one EM step w_k <- w_k g_k (renormalised), which
// never lowers f.  (6) Stop at kkt_gap <= tol or after max_passes passes; every evaluation of (f, g, H) counts as a pass.
#pragma once
#include <math.h>
#include <stdint.h>

#include "predictive.h"

#define CMP_MAXK 8
#define CMP_TAG 0xFFFF0000u
#define CMP_EIG_CUT 1e-10
#define CMP_HALVINGS 6
#define CMP_NACC(K) (1 + (K) + (K) * ((K) + 1) / 2)   // sum log d, K sums of q_k, the upper triangle of sum q_k q_l row by row

// the variates of replicates 2 * pair and 2 * pair + 1 at observation i
PP_HD void cmp_g_pair(PPKey key, int64_t i, uint32_t pair, double& g0, double& g1) {
  const PPBlock bl = pp_block(key, pp_ctr(i, pair, CMP_TAG), 0);
  g0 = -log(bl.u0);
  g1 = -log(bl.u1);
}

PP_HD double cmp_g(uint64_t seed, int64_t b, int64_t i) {
  double g0, g1;
  cmp_g_pair(pp_key(seed), i, (uint32_t)(b >> 1), g0, g1);
  return (b & 1) ? g1 : g0;
}

// p[k] = exp(e[k] - m), returns m = max_k e[k]
template <int K>
PP_HD double cmp_terms(const double (&e)[K], double (&p)[K]) {
  double m = e[0];
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int k = 1; k < K; ++k) m = e[k] > m ? e[k] : m;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int k = 0; k < K; ++k) p[k] = exp(e[k] - m);
  return m;
}

// one observation's contribution to the CMP_NACC(K) sums of a pass at w
template <int K>
PP_HD void cmp_pass_add(const double (&p)[K], const double (&w)[K], double (&a)[CMP_NACC(K)]) {
  double d = 0.0, q[K];
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int k = 0; k < K; ++k) d = fma(w[k], p[k], d);
  const double r = 1.0 / d;
  a[0] += log(d);
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int k = 0; k < K; ++k) { q[k] = p[k] * r; a[1 + k] += q[k]; }
  int at = 1 + K;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int k = 0; k < K; ++k) {
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int l = k; l < K; ++l) { a[at] = fma(q[k], q[l], a[at]); ++at; }
  }
}

// ---- host half: the solver ----------------------------------------------------------------------------------------------------------
// a pass: the CMP_NACC(K) raw sums at w; false on failure (the solver stops and reports it)
typedef bool (*cmp_pass_fn)(void* ctx, const double* w, double* sums);

struct CmpEval { double ld; double g[CMP_MAXK]; double H[CMP_MAXK][CMP_MAXK]; };

inline void cmp_unpack(int K, int64_t N, const double* sums, CmpEval& ev) {
  ev.ld = sums[0];
  for (int k = 0; k < K; ++k) ev.g[k] = sums[1 + k] / (double)N;
  int at = 1 + K;
  for (int k = 0; k < K; ++k)
    for (int l = k; l < K; ++l) { ev.H[k][l] = ev.H[l][k] = -sums[at] / (double)N; ++at; }
}

// x of least norm minimising |A x - b|, A symmetric n x n (n <= CMP_MAXK + 1), by cyclic Jacobi
inline void cmp_min_norm_solve(int n, double A[CMP_MAXK + 1][CMP_MAXK + 1], const double* b, double* x) {
  double V[CMP_MAXK + 1][CMP_MAXK + 1];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i) {
      diag += A[i][i] * A[i][i];
      for (int j = i + 1; j < n; ++j) off += A[i][j] * A[i][j];
    }
    if (off <= 1e-34 * diag || off == 0.0) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  double top = 0.0;
  for (int i = 0; i < n; ++i) top = fabs(A[i][i]) > top ? fabs(A[i][i]) : top;
  for (int i = 0; i < n; ++i) x[i] = 0.0;
  for (int j = 0; j < n; ++j) {
    if (!(fabs(A[j][j]) > CMP_EIG_CUT * top)) continue;
    double proj = 0.0;
    for (int i = 0; i < n; ++i) proj += V[i][j] * b[i];
    proj /= A[j][j];
    for (int i = 0; i < n; ++i) x[i] += V[i][j] * proj;
  }
}

inline void cmp_newton_direction(int K, const double* w, const CmpEval& ev, double* delta) {
  bool free_[CMP_MAXK];
  for (int k = 0; k < K; ++k) free_[k] = w[k] > 0.0 || ev.g[k] > 1.0;
  for (;;) {
    int F[CMP_MAXK], nf = 0;
    for (int k = 0; k < K; ++k) if (free_[k]) F[nf++] = k;
    double A[CMP_MAXK + 1][CMP_MAXK + 1], rhs[CMP_MAXK + 1], x[CMP_MAXK + 1];
    for (int a = 0; a < nf; ++a) {
      for (int c = 0; c < nf; ++c) A[a][c] = ev.H[F[a]][F[c]];
      A[a][nf] = A[nf][a] = 1.0;
      rhs[a] = -ev.g[F[a]];
    }
    A[nf][nf] = 0.0; rhs[nf] = 0.0;
    cmp_min_norm_solve(nf + 1, A, rhs, x);
    for (int k = 0; k < K; ++k) delta[k] = 0.0;
    for (int a = 0; a < nf; ++a) delta[F[a]] = x[a];
    bool stuck = false;
    for (int k = 0; k < K; ++k)
      if (free_[k] && w[k] <= 0.0 && delta[k] <= 0.0) { free_[k] = false; stuck = true; }
    if (!stuck) return;
  }
}

inline double cmp_gap(int K, const CmpEval& ev) {
  double g = ev.g[0];
  for (int k = 1; k < K; ++k) g = ev.g[k] > g ? ev.g[k] : g;
  return g - 1.0;
}

// w[K] (out), *ld = sum_i log d_i at w (f = sum_i m_i + *ld), *gap, *passes.  false: a pass failed.
inline bool cmp_solve(int K, int64_t N, cmp_pass_fn pass, void* ctx, double tol, int max_passes, double* w, double* ld, double* gap, int* passes) {
  double sums[CMP_NACC(CMP_MAXK)];
  CmpEval ev, evn;
  for (int k = 0; k < K; ++k) w[k] = 1.0 / (double)K;
  if (!pass(ctx, w, sums)) return false;
  cmp_unpack(K, N, sums, ev);
  int np = 1;
  for (;;) {
    if (cmp_gap(K, ev) <= tol || np >= max_passes) break;
    double delta[CMP_MAXK], wn[CMP_MAXK];
    cmp_newton_direction(K, w, ev, delta);
    bool any = false, accepted = false;
    for (int k = 0; k < K; ++k) any = any || delta[k] != 0.0;
    if (any) {
      double alpha = 1.0;
      int hit = -1;
      for (int k = 0; k < K; ++k)
        if (delta[k] < 0.0 && -w[k] / delta[k] < alpha) { alpha = -w[k] / delta[k]; hit = k; }
      const double slack = 1e-13 * (fabs(ev.ld) > 1.0 ? fabs(ev.ld) : 1.0);
      for (int h = 0; h < CMP_HALVINGS && np < max_passes; ++h) {
        double tot = 0.0;
        for (int k = 0; k < K; ++k) {
          const double v = w[k] + alpha * delta[k];
          wn[k] = v > 0.0 ? v : 0.0;
        }
        if (h == 0 && hit >= 0) wn[hit] = 0.0;
        for (int k = 0; k < K; ++k) tot += wn[k];
        for (int k = 0; k < K; ++k) wn[k] /= tot;
        if (!pass(ctx, wn, sums)) return false;
        ++np;
        cmp_unpack(K, N, sums, evn);
        if (isfinite(evn.ld) && evn.ld >= ev.ld - slack) {
          for (int k = 0; k < K; ++k) w[k] = wn[k];
          ev = evn;
          accepted = true;
          break;
        }
        alpha *= 0.5;
      }
    }
    if (!accepted && np < max_passes) {
      double tot = 0.0;
      for (int k = 0; k < K; ++k) { wn[k] = w[k] * ev.g[k]; tot += wn[k]; }
      for (int k = 0; k < K; ++k) w[k] = wn[k] / tot;
      if (!pass(ctx, w, sums)) return false;
      ++np;
      cmp_unpack(K, N, sums, ev);
    }
  }
  *ld = ev.ld;
  *gap = cmp_gap(K, ev);
  *passes = np;
  return true;
}
