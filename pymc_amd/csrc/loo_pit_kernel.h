// LOO predictive checks (`az.loo_pit`, the LOO predictive mean and variance per observation) from a SECOND pass over the draws
// (include/nuts_mi355.h, nuts_loo_pit_*).  After nuts_psis_update has seen all S draws, the state of psis.h fixes
// the Pareto-smoothed weight of every draw: psis_fit makes it a record per observation, psis_weight reads the weight of one
// log-likelihood value off the record and the sorted column.  Per batch the second pass evaluates the log-likelihood block, turns
// it into weights, evaluates the replicates of the same draws (predictive_kernel.h) and folds both per observation.  The kernels
// keep the rules of loglik_kernel.h: no atomics; nothing depends on how many draws share the launch or on how the draws were split
// over calls.
//
//   k_psis_fit    a thread per observation, the geometry and the LDS work columns of k_psis_finish: fit = [PSIS_FIT_FIELDS][N]
//   k_loo_weight  a thread per (observation, draw of the batch) over the [nb][N] log-likelihood block: the record's cutoff is one
//                 coalesced read, and only a draw of the tail (about M of S) walks the column for its rank
//   k_loo_fold    a thread per observation folds its column of weights and replicates, in draw order
#pragma once
#include "loglik_kernel.h"

__global__ __launch_bounds__(PSIS_FIN_BLOCK) void k_psis_fit(const double* __restrict__ keep, const double* __restrict__ acc, int64_t N, int K1,
                                                            int64_t S, double* __restrict__ fit) {
  __shared__ double work[PSIS_WORK * PSIS_FIN_BLOCK];
  const int64_t i = (int64_t)blockIdx.x * PSIS_FIN_BLOCK + threadIdx.x;
  if (i >= N) return;
  const PsisFit f = psis_fit(keep + i, N, K1, acc[2 * N + i], acc[3 * N + i], S, work + threadIdx.x, PSIS_FIN_BLOCK);
  fit[i] = f.c; fit[N + i] = f.xc; fit[2 * N + i] = (double)f.tl; fit[3 * N + i] = f.khat; fit[4 * N + i] = f.sigma;
  fit[5 * N + i] = f.logden; fit[6 * N + i] = (double)f.state;
}

// w = [nb][N]: the normalised weight of draw b at observation i (NaN where the fit is degenerate or poisoned)
__global__ __launch_bounds__(LL_BLOCK) void k_loo_weight(const double* __restrict__ ll, int64_t N, const double* __restrict__ fit,
                                                         const double* __restrict__ keep, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= N) return;
  const double v = ll[(int64_t)b * N + i];
  PsisFit f;
  f.c = fit[i]; f.xc = fit[N + i]; f.logden = fit[5 * N + i]; f.state = (int)fit[6 * N + i];
  double out;
  if (f.state != PSIS_FIT_OK) out = NAN;
  else if (!(-v - f.c > f.xc)) out = exp(-v - f.c - f.logden);   // (psis_weight's own first branch: the rest of the record stays unread)
  else {
    f.tl = (int)fit[2 * N + i]; f.khat = fit[3 * N + i]; f.sigma = fit[4 * N + i];
    out = psis_weight(f, keep + i, N, v);
  }
  w[(int64_t)b * N + i] = out;
}

// acc = [6][N]: sum w, sum w^2, sum w [y_rep < y], sum w [y_rep == y], the weighted mean and M2 of y_rep (West 1979: with
// W = sum w so far, mean += (w / W)(x - mean), M2 += w (x - mean_before)(x - mean_after)).  A NaN replicate enters the mean and M2
// of its observation only; a comparison with NaN is false, so the weighted counts never see it (as in k_ppc_fold).  A weight of 0
// while W is still 0 leaves the mean alone.
__global__ __launch_bounds__(LL_BLOCK) void k_loo_fold(const double* __restrict__ w, const double* __restrict__ v, int nb, int64_t N,
                                                       const double* __restrict__ y_obs, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
  double x[LL_B], ww[LL_B];
#pragma unroll
  for (int b = 0; b < LL_B; ++b) {
    x[b] = b < nb ? v[(int64_t)b * N + i] : 0.0;
    ww[b] = b < nb ? w[(int64_t)b * N + i] : 0.0;
  }
  const double y = y_obs[i];
  double W = acc[i], W2 = acc[N + i], p_lt = acc[2 * N + i], p_eq = acc[3 * N + i], mean = acc[4 * N + i], M2 = acc[5 * N + i];
#pragma unroll
  for (int b = 0; b < LL_B; ++b) {
    if (b >= nb) break;
    const double wb = ww[b];
    W += wb;
    W2 = fma(wb, wb, W2);
    p_lt += x[b] < y ? wb : 0.0;
    p_eq += x[b] == y ? wb : 0.0;
    if (!(W == 0.0)) {
      const double dl = x[b] - mean;
      mean = fma(wb / W, dl, mean);
      M2 = fma(wb * dl, x[b] - mean, M2);
    }
  }
  acc[i] = W; acc[N + i] = W2; acc[2 * N + i] = p_lt; acc[3 * N + i] = p_eq; acc[4 * N + i] = mean; acc[5 * N + i] = M2;
}

__global__ __launch_bounds__(LL_BLOCK) void k_loo_init(int64_t N, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[(int64_t)k * N + i] = 0.0;
}
