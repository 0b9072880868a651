// Posterior-predictive replicates of observed factors and dense nodes at a BATCH of positions, and the streaming summaries of
// `az.plot_ppc` / `az.plot_bpv` (include/nuts_mi355.h, nuts_model_predictive / nuts_ppc_*).  The kernels sit beside those of
// loglik_kernel.h and keep their three rules: no atomics; the value of (draw, observation) never depends on how many draws share
// the launch (predictive.h: it is a function of (seed, node, global draw index, observation index) -- unused columns of a ragged
// batch are evaluated and not stored); the host uploads draws in blocks of LL_B.
//
//   k_pp_glm      the row pass of k_ll_glm (the same body, ll_glm_pass) storing the linear predictor eta[b][N] into the stage
//   k_pp_rows     the body of k_ll_rows storing eta; k_pp_rows_y the same indexing storing the rows' y (int8, tile order) as doubles
//   k_pp_draw     a thread per (draw, observation): the stage, in place, from eta to a variate of the node's family -- the rejection
//                 loops of the gamma and Poisson generators live here, not in the 250-register row pass
//   k_pp_factor   an element-wise factor: prog_forward + pp_draw per (draw, element); a failed NUTS_E_CHECK marks the draw, k_pp_fill
//                 then writes NaN over its row (the flag-vector protocol of k_ll_factor / k_ll_fill)
//   k_pp_mix      the marginal Normal mixture, a thread per (draw, row)
//   k_ppc_fold    a thread per observation folds its column of the [nb][N] block, in draw order, into (mean, M2, #{y_rep < y},
//                 #{y_rep == y}); the workgroup's (sum, sum of squares, min, max) over ITS observations of every draw go to a fixed
//                 slot part[block][draw][4]; k_ppc_stats adds the slots of a draw in one fixed order.  A draw's four numbers depend on
//                 N and on nothing else.
#pragma once
#include "loglik_kernel.h"
#include "predictive.h"

static_assert(PP_D_NORMAL == NUTS_D_NORMAL && PP_D_STUDENTT == NUTS_D_STUDENTT && PP_D_BERNOULLI_LOGIT == NUTS_D_BERNOULLI_LOGIT &&
              PP_D_TRUNCNORMAL == NUTS_D_TRUNCNORMAL && PP_D_GAMMA == NUTS_D_GAMMA && PP_D_POISSON == NUTS_D_POISSON &&
              PP_D_DERIVED == NUTS_D_DERIVED, "predictive.h restates the distribution codes of nuts_mi355.h");

struct PPAddr { PPKey key; uint32_t tag, s0; };   // s0: the global index of the batch's first draw

template <int LPR, int CH, int B>
__global__ __launch_bounds__(GLM_BLOCK, 2) void k_pp_glm(GlmDev gm, const double* __restrict__ Beta, const double* __restrict__ sc, int nb,
                                                        double* __restrict__ out) {
  ll_glm_pass<LPR, CH, B, true>(gm, Beta, sc, nb, nullptr, out);
}

__global__ __launch_bounds__(LL_BLOCK) void k_pp_rows(ModelDev md, const double* __restrict__ beta, int span, int LW, double* __restrict__ out) {
  ll_rows_body<true, false>(md, beta, span, LW, out);
}
__global__ __launch_bounds__(LL_BLOCK) void k_pp_rows_y(ModelDev md, const double* __restrict__ beta, int span, int LW, double* __restrict__ out) {
  ll_rows_body<false, true>(md, beta, span, LW, out);
}

// dist: NUTS_D_NORMAL (eta, sigma of the draw: sc[4 b + 1]), NUTS_D_BERNOULLI_LOGIT (eta) or NUTS_D_POISSON (mu = exp(eta))
__global__ __launch_bounds__(LL_BLOCK) void k_pp_draw(double* __restrict__ stage, int64_t N, int dist, const double* __restrict__ sc, PPAddr ad) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= N) return;
  const double eta = stage[(int64_t)b * N + i];
  const double a1 = dist == NUTS_D_POISSON ? exp(eta) : eta;
  const double a2 = dist == NUTS_D_NORMAL ? sc[4 * b + 1] : 0.0;
  stage[(int64_t)b * N + i] = pp_draw(dist, 0.0, a1, a2, 0.0, ad.key, pp_ctr(i, ad.s0 + (uint32_t)b, ad.tag));
}

__global__ __launch_bounds__(LL_BLOCK) void k_pp_factor(ModelDev md, const double* __restrict__ q, int fi, double* __restrict__ out,
                                                        int32_t* __restrict__ dead, PPAddr ad) {
  const Prog pg = prog_view(md, md.prog);
  const nuts_factor& f = pg.factors[fi];
  const int li = blockIdx.x * LL_BLOCK + threadIdx.x, b = blockIdx.y;
  if (li >= f.size) return;
  const QView qv = ll_view(q + (int64_t)b * md.n);
  double tv[NUTS_MAX_FACTOR_INSTR];
  ProgFwd o;
  prog_forward(pg, qv, f, li, -1, 0.0, tv, o);
  if (o.pdead) dead[b] = 1;   // (every writer stores the same value)
  out[(int64_t)b * f.size + li] = pp_draw(f.dist, f.konst, o.a[1], o.a[2], o.a[3], ad.key, pp_ctr(li, ad.s0 + (uint32_t)b, ad.tag));
}

__global__ __launch_bounds__(LL_BLOCK) void k_pp_fill(double* __restrict__ out, int64_t size, const int32_t* __restrict__ dead) {
  const int64_t li = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (li < size && dead[b]) out[(int64_t)b * size + li] = NAN;
}

// y_obs of a factor: its argument 0 (observed data: it does not depend on the position it is evaluated at)
__global__ __launch_bounds__(LL_BLOCK) void k_pp_factor_y(ModelDev md, const double* __restrict__ q, int fi, double* __restrict__ out) {
  const Prog pg = prog_view(md, md.prog);
  const nuts_factor& f = pg.factors[fi];
  const int li = blockIdx.x * LL_BLOCK + threadIdx.x;
  if (li >= f.size) return;
  const QView qv = ll_view(q);
  double tv[NUTS_MAX_FACTOR_INSTR];
  ProgFwd o;
  prog_forward(pg, qv, f, li, -1, 0.0, tv, o);
  out[li] = o.a[0];
}

__global__ __launch_bounds__(MIX_BLOCK) void k_pp_mix(ModelDev md, const double* __restrict__ q, double* __restrict__ out, PPAddr ad) {
  const MixDev& mx = md.mix;
  const int b = blockIdx.y;
  const QView qv = ll_view(q + (int64_t)b * md.n);
  __shared__ double s_par[3][MIX_MAXK];   // mu, sigma, w
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid >> 6, K = mx.K;
  if (w == 0) {
    double mu, sg, lw, lse;
    mix_params(mx, qv, lane & (MIX_MAXK - 1), mu, sg, lw, lse);
    if (lane < K) { s_par[0][lane] = mu; s_par[1][lane] = sg; s_par[2][lane] = exp(lw); }
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * MIX_BLOCK + tid;
  if (i >= mx.N) return;
  out[(int64_t)b * mx.N + i] = pp_mixture(K, s_par[0], s_par[1], s_par[2], ad.key, pp_ctr(i, ad.s0 + (uint32_t)b, ad.tag));
}

// ---- streaming summaries -------------------------------------------------------------------------------------------------------
// NaN replicates (an element with invalid parameters, the row of a draw whose check failed) are NOT hidden: min and max propagate
// them as the sums do, so all four numbers of such a draw are NaN; the observation's mean and M2 become NaN for good, and its two
// counts, which a NaN never enters, are to be read as undefined wherever mean_i is NaN (predictive.ppc_from_accumulators does).
__device__ __forceinline__ double pp_min(double a, double b) { return (a != a || b != b) ? NAN : fmin(a, b); }
__device__ __forceinline__ double pp_max(double a, double b) { return (a != a || b != b) ? NAN : fmax(a, b); }
// acc = [4][N]: mean, M2 (Welford), #{y_rep < y}, #{y_rep == y} (counts as doubles); nullptr: only the per-draw partials (T of y_obs
// itself).  part = [gridDim.x][LL_B][4]: (sum, sum of squares, min, max) of the workgroup's observations at draw b; rows beyond N
// carry the identities.  Lanes are reduced by a fixed butterfly, the waves of the workgroup in wave order.
__global__ __launch_bounds__(LL_BLOCK) void k_ppc_fold(const double* __restrict__ v, int nb, int64_t N, int64_t count, const double* __restrict__ y_obs,
                                                       double* __restrict__ acc, double* __restrict__ part) {
  __shared__ double s_w[LL_BLOCK / WAVE][LL_B][4];
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  const bool live = i < N;
  double x[LL_B];
#pragma unroll
  for (int b = 0; b < LL_B; ++b) x[b] = live && b < nb ? v[(int64_t)b * N + i] : 0.0;
  if (live && acc) {
    const double y = y_obs[i];
    double mean = acc[i], M2 = acc[N + i], n_lt = acc[2 * N + i], n_eq = acc[3 * N + i];
#pragma unroll
    for (int b = 0; b < LL_B; ++b) {
      if (b >= nb) break;
      const double k = (double)(count + b + 1);
      const double dl = x[b] - mean;
      mean += dl / k;
      M2 = fma(dl, x[b] - mean, M2);
      n_lt += x[b] < y ? 1.0 : 0.0;
      n_eq += x[b] == y ? 1.0 : 0.0;
    }
    acc[i] = mean; acc[N + i] = M2; acc[2 * N + i] = n_lt; acc[3 * N + i] = n_eq;
  }
#pragma unroll
  for (int b = 0; b < LL_B; ++b) {
    double s = live ? x[b] : 0.0, ss = live ? x[b] * x[b] : 0.0, mn = live ? x[b] : INFINITY, mx = live ? x[b] : -INFINITY;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      s += __shfl_xor(s, o, WAVE); ss += __shfl_xor(ss, o, WAVE);
      mn = pp_min(mn, __shfl_xor(mn, o, WAVE)); mx = pp_max(mx, __shfl_xor(mx, o, WAVE));
    }
    if (lane == 0) { s_w[w][b][0] = s; s_w[w][b][1] = ss; s_w[w][b][2] = mn; s_w[w][b][3] = mx; }
  }
  __syncthreads();
  if (threadIdx.x < LL_B) {
    const int b = threadIdx.x;
    double s = s_w[0][b][0], ss = s_w[0][b][1], mn = s_w[0][b][2], mx = s_w[0][b][3];
#pragma unroll
    for (int ww = 1; ww < LL_BLOCK / WAVE; ++ww) { s += s_w[ww][b][0]; ss += s_w[ww][b][1]; mn = pp_min(mn, s_w[ww][b][2]); mx = pp_max(mx, s_w[ww][b][3]); }
    double* p = part + ((int64_t)blockIdx.x * LL_B + b) * 4;
    p[0] = s; p[1] = ss; p[2] = mn; p[3] = mx;
  }
}

// One workgroup per draw b < nb: thread t adds the slots of the workgroups t, t + LL_BLOCK, ... in that order, then the threads'
// totals are combined as k_ppc_fold combines lanes and waves.  T = the draw's (sum, sum of squares, min, max).
__global__ __launch_bounds__(LL_BLOCK) void k_ppc_stats(const double* __restrict__ part, int64_t nblk, double* __restrict__ T) {
  __shared__ double s_w[LL_BLOCK / WAVE][4];
  const int b = blockIdx.x, lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  double s = 0.0, ss = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int64_t k = threadIdx.x; k < nblk; k += LL_BLOCK) {
    const double* p = part + (k * LL_B + b) * 4;
    s += p[0]; ss += p[1]; mn = pp_min(mn, p[2]); mx = pp_max(mx, p[3]);
  }
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    s += __shfl_xor(s, o, WAVE); ss += __shfl_xor(ss, o, WAVE);
    mn = pp_min(mn, __shfl_xor(mn, o, WAVE)); mx = pp_max(mx, __shfl_xor(mx, o, WAVE));
  }
  if (lane == 0) { s_w[w][0] = s; s_w[w][1] = ss; s_w[w][2] = mn; s_w[w][3] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int ww = 1; ww < LL_BLOCK / WAVE; ++ww) { s += s_w[ww][0]; ss += s_w[ww][1]; mn = pp_min(mn, s_w[ww][2]); mx = pp_max(mx, s_w[ww][3]); }
    T[4 * b + 0] = s; T[4 * b + 1] = ss; T[4 * b + 2] = mn; T[4 * b + 3] = mx;
  }
}

__global__ __launch_bounds__(LL_BLOCK) void k_ppc_init(int64_t N, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
  acc[i] = 0.0; acc[N + i] = 0.0; acc[2 * N + i] = 0.0; acc[3 * N + i] = 0.0;
}
