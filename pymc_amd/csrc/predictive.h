// Posterior-predictive variates: one random value per (draw, observation) of an observed node, from a COUNTER-BASED generator, so
// that the value of (draw s, observation i) is a function of (seed, node, s, i) and nothing else -- not of the batch the draw
// travelled in, of the split of the draws over calls, of the kernel route or of the layout of X.  A header the system C++ compiler
// and hipcc both accept: k_pp_draw / k_pp_factor / k_pp_mix (predictive_kernel.h) call it on the device, tests/predictive_check.cpp
// wraps it in a stand-alone host program that tests/test_predictive_host.py holds to the NumPy restatement
// (tests/predictive_reference.py).
//
// Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11).
//   key     = (seed low 32, seed high 32)
//   counter = (i low 32, i high 32, s, tag),  tag = kind << 30 | (index & 0x3fff) << 16 | t
// i: the index the node's log-likelihood kernel uses (logit rows: the spec's group-sorted order); s: the GLOBAL draw index; (kind,
// index): the node (NUTS_LL_*); t < 65536 numbers the 128-bit BLOCKS one variate consumes.  A block (w0, w1, w2, w3) gives two
// doubles:  u0 from (w_lo, w_hi) = (w0, w1), u1 from (w2, w3),
//   u = ((w_hi >> 5) 2^26 + (w_lo >> 6) + 0.5) 2^-53,
// never 0, so log(u) is always finite; the smallest is 2^-54.  (k + 0.5 of the 53-bit integer k rounds to even from 2^52 on: the ONE
// value k = 2^53 - 1 gives u = 1.0, probability 2^-53 -- a Laplace variate is +inf there, every other family stays finite.)
//
// Blocks per family (z(t) = sqrt(-2 log u0) cos(2 pi u1) of block t, Box-Muller; G(a; t0) the Marsaglia-Tsang gamma below):
//   Normal, HalfNormal, LogNormal          z(0):  mu + sigma z, sigma |z|, exp(mu + sigma z)
//   Cauchy                                 u0 of block 0:  alpha + beta tan(pi (u - 1/2))
//   HalfCauchy                             u0 of block 0:  beta tan(pi u / 2)
//   Laplace                                u0 of block 0:  u < 1/2 ? mu + b log(2 u) : mu - b log(2 (1 - u))
//   Exponential                            u0 of block 0:  -log(u) / lam  (the survival function inverted)
//   Uniform                                u0 of block 0:  lower + (upper - lower) u
//   Bernoulli, Bernoulli-logit             u0 of block 0:  u < p, p = sigmoid(eta)
//   Gamma, InvGamma                        G(alpha; 0) / beta,  beta / G(alpha; 0)
//   Beta                                   g1 = G(alpha; 0), g2 = G(beta; 64):  g1 / (g1 + g2)
//   StudentT                               g = G(nu / 2; 0), z(128):  mu + sigma z / sqrt(2 g / nu)
//   Poisson, mu < 10                       u0 of block 0: sequential search, k = 0, p = s = exp(-mu); while u > s: k += 1, p *= mu / k,
//                                          s += p (at most PP_POIS_KMAX steps)
//   Poisson, mu >= 10                      Hormann's PTRS ("The transformed rejection method for generating Poisson random variables",
//                                          1993): attempt j < 64 takes (U, V) = (u0 - 1/2, u1) of block j; NaN after 64 rejections
//   G(a; t0), Marsaglia & Tsang, "A simple method for generating gamma variables", 2000 (without the squeeze): a' = a < 1 ? a + 1 : a,
//     d = a' - 1/3, c = 1 / sqrt(9 d); attempt j < 32 takes x = z(t0 + 2 j) and (u, u') = (u0, u1) of block t0 + 2 j + 1;
//     v = (1 + c x)^3; accepted when v > 0 and log u < x^2 / 2 + d - d v + d log v:  g = d v, times u'^(1 / a) when a < 1 (u' is
//     independent of the test); NaN after 32 rejections.  One gamma spans 64 blocks: a second one starts at 64.
//   Normal mixture (predictive_kernel.h)   u0 of block 0 picks the component (the first k with u < w_0 + ... + w_k, the last one
//                                          catches the rest), z(1) is its normal
// Invalid parameters -- the conditions of KILL_PARAM in dist_eval_body (model_dev.h) -- give NaN for that element.
#pragma once
#include <math.h>
#include <stdint.h>

#include "scalar_math.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PP_HD __host__ __device__ __forceinline__
#else
#define PP_HD inline
#endif

#define PP_GAMMA_TRIES 32
#define PP_GAMMA_BLOCKS (2 * PP_GAMMA_TRIES)
#define PP_PTRS_TRIES 64
#define PP_POIS_KMAX 1000   // the search of the small-mean Poisson stops here (s has long stopped moving: exp(-10) 10^k / k! < 1e-300)
#define PP_T_BLOCK 128      // StudentT: the block of its normal, after the gamma's range

// distribution codes of include/nuts_mi355.h (NUTS_D_*), restated so that the header stands alone on the host
enum {
  PP_D_NORMAL = 0, PP_D_HALFNORMAL = 1, PP_D_CAUCHY = 2, PP_D_HALFCAUCHY = 3, PP_D_STUDENTT = 4, PP_D_BETA = 5, PP_D_EXPONENTIAL = 6,
  PP_D_UNIFORM = 7, PP_D_BERNOULLI_LOGIT = 8, PP_D_LOGNORMAL = 9, PP_D_BERNOULLI = 10, PP_D_TRUNCNORMAL = 11, PP_D_POTENTIAL = 12,
  PP_D_BINOMIAL = 13, PP_D_GAMMA = 14, PP_D_INVGAMMA = 15, PP_D_LAPLACE = 16, PP_D_POISSON = 17, PP_D_DERIVED = 18
};

struct PPKey { uint32_t k0, k1; };
struct PPCtr { uint32_t c0, c1, c2, c3; };   // c3: the tag with t = 0
struct PPBlock { double u0, u1; };

PP_HD PPKey pp_key(uint64_t seed) { return PPKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }

// tag of node (kind, index), t = 0; false when the index does not fit its 14 bits (or the kind its 2)
PP_HD bool pp_tag(int32_t kind, int32_t index, uint32_t* tag) {
  if (kind < 0 || kind > 3 || index < 0 || index > 0x3fff) return false;
  *tag = (uint32_t)kind << 30 | (uint32_t)index << 16;
  return true;
}
PP_HD PPCtr pp_ctr(int64_t i, uint32_t s, uint32_t tag) { return PPCtr{(uint32_t)(uint64_t)i, (uint32_t)((uint64_t)i >> 32), s, tag}; }

PP_HD void pp_philox(PPKey key, PPCtr ctr, uint32_t out[4]) {
  uint32_t c0 = ctr.c0, c1 = ctr.c1, c2 = ctr.c2, c3 = ctr.c3, k0 = key.k0, k1 = key.k1;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

PP_HD double pp_u53(uint32_t lo, uint32_t hi) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 0.5) * 1.1102230246251565404e-16;   // 2^26, 2^-53
}

PP_HD PPBlock pp_block(PPKey key, PPCtr ctr, uint32_t t) {
  uint32_t w[4];
  ctr.c3 |= t;
  pp_philox(key, ctr, w);
  return PPBlock{pp_u53(w[0], w[1]), pp_u53(w[2], w[3])};
}

PP_HD double pp_normal(PPKey key, PPCtr ctr, uint32_t t) {
  const PPBlock b = pp_block(key, ctr, t);
  return sqrt(-2.0 * log(b.u0)) * cos(6.283185307179586477 * b.u1);
}

// standard gamma of shape a > 0 from the blocks t0 .. t0 + PP_GAMMA_BLOCKS - 1
PP_HD double pp_gamma(double a, PPKey key, PPCtr ctr, uint32_t t0) {
  const double a1 = a < 1.0 ? a + 1.0 : a;
  const double d = a1 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  for (uint32_t j = 0; j < PP_GAMMA_TRIES; ++j) {
    const double x = pp_normal(key, ctr, t0 + 2 * j);
    const PPBlock b = pp_block(key, ctr, t0 + 2 * j + 1);
    const double w = 1.0 + c * x, v = w * w * w;
    if (v > 0.0 && log(b.u0) < 0.5 * x * x + d - d * v + d * log(v)) {
      const double g = d * v;
      return a < 1.0 ? g * exp(log(b.u1) / a) : g;
    }
  }
  return NAN;
}

PP_HD double pp_poisson(double mu, PPKey key, PPCtr ctr) {
  if (mu < 10.0) {
    const double u = pp_block(key, ctr, 0).u0;
    double k = 0.0, p = exp(-mu), s = p;
    while (u > s && k < (double)PP_POIS_KMAX) { k += 1.0; p *= mu / k; s += p; }
    return k;
  }
  const double smu = sqrt(mu), b = 0.931 + 2.53 * smu, a = -0.059 + 0.02483 * b;
  const double inv_alpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0), lmu = log(mu);
  for (uint32_t j = 0; j < PP_PTRS_TRIES; ++j) {
    const PPBlock bl = pp_block(key, ctr, j);
    const double U = bl.u0 - 0.5, V = bl.u1, us = 0.5 - fabs(U);
    const double k = floor((2.0 * a / us + b) * U + mu + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(inv_alpha) - log(a / (us * us) + b) <= -mu + k * lmu - lgamma(k + 1.0)) return k;
  }
  return NAN;
}

// true for the families pp_draw covers
PP_HD bool pp_family_ok(int dist) {
  return dist != PP_D_TRUNCNORMAL && dist != PP_D_POTENTIAL && dist != PP_D_BINOMIAL && dist != PP_D_DERIVED && dist >= 0 && dist <= PP_D_POISSON;
}

// One variate of family `dist` with the factor's arguments 1 .. 3 (argument 0, the observed value, is not read) and its constant.
PP_HD double pp_draw(int dist, double konst, double a1, double a2, double a3, PPKey key, PPCtr ctr) {
  (void)konst;
  switch (dist) {
    case PP_D_NORMAL: return !(a2 > 0) ? NAN : a1 + a2 * pp_normal(key, ctr, 0);
    case PP_D_HALFNORMAL: return !(a1 > 0) ? NAN : a1 * fabs(pp_normal(key, ctr, 0));
    case PP_D_LOGNORMAL: return !(a2 > 0) ? NAN : exp(a1 + a2 * pp_normal(key, ctr, 0));
    case PP_D_CAUCHY: return !(a2 > 0) ? NAN : a1 + a2 * tan(3.141592653589793238 * (pp_block(key, ctr, 0).u0 - 0.5));
    case PP_D_HALFCAUCHY: return !(a1 > 0) ? NAN : a1 * tan(1.570796326794896619 * pp_block(key, ctr, 0).u0);
    case PP_D_LAPLACE: {
      if (!(a2 > 0)) return NAN;
      const double u = pp_block(key, ctr, 0).u0;
      return u < 0.5 ? a1 + a2 * log(2.0 * u) : a1 - a2 * log(2.0 * (1.0 - u));
    }
    case PP_D_EXPONENTIAL: return !(a1 > 0) ? NAN : -log(pp_block(key, ctr, 0).u0) / a1;
    case PP_D_UNIFORM: return !(a1 <= a2) ? NAN : a1 + (a2 - a1) * pp_block(key, ctr, 0).u0;
    case PP_D_BERNOULLI: return !(a1 >= 0 && a1 <= 1) ? NAN : (pp_block(key, ctr, 0).u0 < a1 ? 1.0 : 0.0);
    case PP_D_BERNOULLI_LOGIT: return a1 != a1 ? NAN : (pp_block(key, ctr, 0).u0 < sigmoid_d(a1) ? 1.0 : 0.0);
    case PP_D_GAMMA: {
      const double be = 1.0 / (1.0 / a2);   // (as the density takes it)
      return !(a1 > 0 && be > 0) ? NAN : pp_gamma(a1, key, ctr, 0) / be;
    }
    case PP_D_INVGAMMA: return !(a1 > 0 && a2 > 0) ? NAN : a2 / pp_gamma(a1, key, ctr, 0);
    case PP_D_BETA: {
      if (!(a1 > 0 && a2 > 0)) return NAN;
      const double g1 = pp_gamma(a1, key, ctr, 0), g2 = pp_gamma(a2, key, ctr, PP_GAMMA_BLOCKS);
      return g1 / (g1 + g2);
    }
    case PP_D_STUDENTT: {
      if (!(a1 > 0 && a3 > 0)) return NAN;
      const double g = pp_gamma(0.5 * a1, key, ctr, 0), z = pp_normal(key, ctr, PP_T_BLOCK);
      return a2 + a3 * z / sqrt(2.0 * g / a1);
    }
    case PP_D_POISSON: return !(a1 >= 0) ? NAN : pp_poisson(a1, key, ctr);
    default: return NAN;
  }
}

// marginal Normal mixture: w[k] the weights, k < K
PP_HD double pp_mixture(int K, const double* mu, const double* sigma, const double* w, PPKey key, PPCtr ctr) {
  const double u = pp_block(key, ctr, 0).u0;
  int k = 0;
  double c = w[0];
  while (k < K - 1 && !(u < c)) { ++k; c += w[k]; }
  return mu[k] + sigma[k] * pp_normal(key, ctr, 1);
}
