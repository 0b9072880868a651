// Prior draws of the free variables at a BATCH of draws (include/nuts_mi355.h, nuts_model_prior): ONE launch per level of the
// ancestral order (engine.hip, prior_build_plan), the levels separated by stream order.  The rules of predictive_kernel.h hold: no
// atomics, no traffic between workgroups, and the value of (draw, variable, element) is a function of (seed, variable, global draw
// number, element) and of the parents' values at that draw (prior.h) -- not of the batch the draw travelled in.
//
//   k_prior_level  grid (threads of the level in workgroups of PRIOR_BLOCK, draws of the batch).  A thread finds its variable in the
//                  level's table by its running element count, evaluates the prior factor's arguments at the draw's row of q
//                  through the ordinary view (prog_forward: the earlier levels are there already, and the view applies
//                  transform_x), draws from the family with arguments 1 .. 3 (pp_draw), applies the forward transform and stores
//                  into q[b][offset + i].  The mixture node's Dirichlet weights are ONE thread per draw (K <= MIX_MAXK).
//                  Invalid parameters, and a failed NUTS_E_CHECK of the factor's program at that element, give NaN for the element;
//                  its descendants become NaN through the arithmetic.
#pragma once
#include "loglik_kernel.h"
#include "prior.h"

static_assert(PRIOR_TR_NONE == NUTS_TR_NONE && PRIOR_TR_LOG == NUTS_TR_LOG && PRIOR_TR_LOGODDS == NUTS_TR_LOGODDS &&
              PRIOR_TR_INTERVAL == NUTS_TR_INTERVAL && PRIOR_MAXK == MIX_MAXK, "prior.h restates the codes of nuts_mi355.h and model_dev.h");

#define PRIOR_BLOCK 256

// q: the batch's first row (rows md.n apart), read AND written (no __restrict__: the view aliases it); tab [nvar]; total: the threads
// of the level; s0: the global number of the batch's first draw
__global__ __launch_bounds__(PRIOR_BLOCK) void k_prior_level(ModelDev md, double* q, const PriorVar* __restrict__ tab, int nvar, int total,
                                                            PPKey key, uint32_t s0) {
  const int e = blockIdx.x * PRIOR_BLOCK + threadIdx.x, b = blockIdx.y;
  if (e >= total) return;
  int lo = 0, hi = nvar - 1;   // the last variable whose start <= e
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].start <= e) lo = mid; else hi = mid - 1;
  }
  const PriorVar pv = tab[lo];
  const int li = e - pv.start;
  double* row = q + (int64_t)b * md.n;
  const uint32_t s = s0 + (uint32_t)b, tag = (uint32_t)pv.index << 16;
  if (pv.factor < 0) {
    double y[PRIOR_MAXK];
    prior_dirichlet(md.mix.K, md.mix.alpha, key, s, tag, y, nullptr);
    for (int k = 0; k < pv.size; ++k) row[pv.offset + k] = y[k];
    return;
  }
  if (li >= pv.size) return;
  const Prog pg = prog_view(md, md.prog);
  const nuts_factor& f = pg.factors[pv.factor];
  const QView qv = ll_view(row);
  double tv[NUTS_MAX_FACTOR_INSTR];
  ProgFwd o;
  prog_forward(pg, qv, f, li, -1, 0.0, tv, o);
  const double x = o.pdead ? NAN : pp_draw(f.dist, f.konst, o.a[1], o.a[2], o.a[3], key, prior_ctr(li, s, tag));
  row[pv.offset + li] = prior_forward(pv.transform, pv.lower, pv.upper, x);
}
