// Prior draws: one random value per (draw, element) of a FREE VARIABLE from the factor that is its prior, then the forward
// transform into the unconstrained position the engine samples in -- what `pm.sample_prior_predictive` does ahead of the data's
// replicates (nuts_model_prior, include/nuts_mi355.h; k_prior_level, prior_kernel.h).  A header the system C++ compiler and hipcc
// both accept, as predictive.h is: tests/prior_check.cpp wraps it in a stand-alone host program that tests/test_prior_host.py holds
// to the NumPy restatement (tests/prior_reference.py).
//
// The generator, the variates and their BLOCK TABLE are those of predictive.h (Philox4x32-10, u53, Box-Muller, Marsaglia-Tsang:
// the table in that header's opening comment says which blocks t a family consumes).  Only the ADDRESS differs:
//   key     = pp_key(seed) = (seed low 32, seed high 32)
//   counter = (i low 32, i high 32 | 0x80000000, s, index << 16 | t)
// i: the element within the variable; s: the GLOBAL draw number (draw0 + position in the call); index: the variable's place in
// nuts_model_spec.vars (<= 0x3fff); t < 65536 the block.  Bit 63 of i is SET.  An observation index is an int64 that is never
// negative, so no counter of an observed node (predictive.h: (i low, i high, s, kind << 30 | index << 16 | t)) has bit 31 of its
// second word set: a prior stream never coincides with the stream of an observed node under the same seed, whatever `kind` and
// `index` are -- the replicates drawn AT a prior draw are independent of it.
//
// Forward transforms, the inverses of transform_x (model_dev.h; pymc/logprob/transforms.py:880-891, 1017-1088 `forward`):
//   log       log(x)
//   logodds   log(x) - log1p(-x)
//   interval  the same of (x - lower) / (upper - lower)
//   none      x
// A constrained draw ON the boundary maps to -inf / +inf and one outside it to NaN; neither is clamped (the caller counts them).
//
// The mixture node's Dirichlet weights (w ~ Dirichlet(alpha) under PyMC's simplex transform; the node owns the prior, the value
// variable has no factor): g_k = G(alpha_k; 0) at element k, w = g / sum g with the sum in index order, then
// SimplexTransform.forward (logprob/transforms.py:1091-1100): y = log w, the K - 1 values y[:-1] - mean(y) -- what mix_params
// (mixture_kernel.h) inverts as w = softmax([y, -sum(y)]).
#pragma once
#include "predictive.h"

#define PRIOR_MAXK 16          // components of the mixture node (MIX_MAXK, model_dev.h)
#define PRIOR_INDEX_MAX 0x3fff

// transform codes of include/nuts_mi355.h (NUTS_TR_*), restated so that the header stands alone on the host
enum { PRIOR_TR_NONE = 0, PRIOR_TR_LOG = 1, PRIOR_TR_LOGODDS = 2, PRIOR_TR_INTERVAL = 3 };

// One variable of a level of the ancestral order, as the device holds it (prior_kernel.h).
struct PriorVar {
  int32_t factor;     // index of the prior factor; -1: the mixture node's Dirichlet weights (one thread per draw)
  int32_t index;      // the variable's place in the spec: the counter's tag
  int32_t offset, size, transform;
  int32_t start;      // threads of the level in front of this variable (the running element count)
  double lower, upper;
};

// tag of variable `index`, t = 0; false when the index does not fit its 14 bits
PP_HD bool prior_tag(int32_t index, uint32_t* tag) {
  if (index < 0 || index > PRIOR_INDEX_MAX) return false;
  *tag = (uint32_t)index << 16;
  return true;
}
PP_HD PPCtr prior_ctr(int64_t i, uint32_t s, uint32_t tag) {
  return PPCtr{(uint32_t)(uint64_t)i, (uint32_t)((uint64_t)i >> 32) | 0x80000000u, s, tag};
}

// true for the families a prior can be drawn from: what pp_draw covers, less the discrete ones
PP_HD bool prior_family_ok(int dist) {
  return pp_family_ok(dist) && dist != PP_D_BERNOULLI && dist != PP_D_BERNOULLI_LOGIT && dist != PP_D_POISSON;
}

PP_HD double prior_logit(double p) { return log(p) - log1p(-p); }
PP_HD double prior_forward(int transform, double lower, double upper, double x) {
  switch (transform) {
    case PRIOR_TR_LOG: return log(x);
    case PRIOR_TR_LOGODDS: return prior_logit(x);
    case PRIOR_TR_INTERVAL: return prior_logit((x - lower) / (upper - lower));
    default: return x;
  }
}

// y[0 .. K - 2]: the simplex-transformed value of one Dirichlet(alpha) draw, 3 <= K <= PRIOR_MAXK; w[0 .. K - 1] (may be null): the
// weights themselves.  A concentration that is not positive makes every element NaN.
PP_HD void prior_dirichlet(int K, const double* alpha, PPKey key, uint32_t s, uint32_t tag, double* y, double* w) {
  double g[PRIOR_MAXK];
  double sum = 0.0;
  for (int k = 0; k < K; ++k) {
    g[k] = !(alpha[k] > 0) ? NAN : pp_gamma(alpha[k], key, prior_ctr(k, s, tag), 0);
    sum += g[k];
  }
  double ly = 0.0;
  for (int k = 0; k < K; ++k) {
    const double wk = g[k] / sum;
    if (w) w[k] = wk;
    g[k] = log(wk);
    ly += g[k];
  }
  const double mean = ly / (double)K;
  for (int k = 0; k < K - 1; ++k) y[k] = g[k] - mean;
}
