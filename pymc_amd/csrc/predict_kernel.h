// Predictions at new data (include/nuts_mi355.h, nuts_model_predict_moments / nuts_pred_*): per (draw, observation) the conditional
// mean m and variance v of the node's family (predict.h pd_moments / pd_mixture) and, where held-out values exist, the log-density
// lp of the held-out value; per observation the fold of those over the draws (predict.h pd_fold), so that no draws x observations
// matrix exists.  The kernels sit beside those of loglik_kernel.h / predictive_kernel.h and keep their three rules: no atomics; the
// value of (draw, observation) never depends on how many draws share the launch (a fold walks its column of the batch in draw
// order, reading nothing of the other columns); the host uploads draws in blocks of LL_B.
//
//   k_pd_fold_eta      the GLM node and the logit rows: the stage eta[nb][N] was written by k_pp_glm / k_pp_rows (X is read once per
//                      batch); a thread per observation forms (m, v, lp) of each draw from eta and the draw's scalars sc -- lp through
//                      glm_row / logit_row, the functions ll_glm_pass / ll_rows_body call -- and folds them in draw order
//   k_pd_flags         an element-wise factor: dead[b] = 1 when a parameter check failed at draw b (the protocol of k_ll_factor)
//   k_pd_fold_factor   a thread per element loops over the batch's draws: prog_forward, pd_moments, dist_eval_v, the fold in
//                      registers; a dead draw folds (NaN, NaN, -inf) for every element of the factor
//   k_pd_fold_mix      the marginal mixture: the components of every draw of the batch in LDS, a thread per row
//   k_pd_moments_*     the same three sources storing mean[nb][N] (and var[nb][N]) instead of folding
// acc = [PD_ACC_ROWS][N]: the rows of PDAcc.  Per draw a fold reads 8 bytes of the stage per observation (none for a factor or the
// mixture) and, per batch, reads and writes the six rows: 8 + 96 / LL_B bytes per (draw, observation) in a full batch.
#pragma once
#include "predict.h"
#include "predictive_kernel.h"

static_assert(PP_D_BINOMIAL == NUTS_D_BINOMIAL && PP_D_BERNOULLI == NUTS_D_BERNOULLI && PP_D_LOGNORMAL == NUTS_D_LOGNORMAL &&
              PP_D_INVGAMMA == NUTS_D_INVGAMMA && PP_D_LAPLACE == NUTS_D_LAPLACE, "predict.h reads the distribution codes of nuts_mi355.h");

__device__ __forceinline__ PDAcc pd_acc_load(const double* __restrict__ acc, int64_t N, int64_t i) {
  return PDAcc{acc[i], acc[N + i], acc[2 * N + i], acc[3 * N + i], acc[4 * N + i], acc[5 * N + i]};
}
__device__ __forceinline__ void pd_acc_store(double* __restrict__ acc, int64_t N, int64_t i, const PDAcc& a) {
  acc[i] = a.mean; acc[N + i] = a.M2; acc[2 * N + i] = a.vbar; acc[3 * N + i] = a.lmax; acc[4 * N + i] = a.lsum; acc[5 * N + i] = a.count;
}

__global__ __launch_bounds__(LL_BLOCK) void k_pd_init(int64_t N, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
  pd_acc_store(acc, N, i, pd_acc_init());
}

// ---- a. GLM node and logit rows: from the stage of linear predictors --------------------------------------------------------------
// family: NUTS_GLM_* (the logit rows are NUTS_GLM_BERNOULLI); sc[4 b + ..] = {intercept, sigma, 1 / sigma, log sigma} of draw b
__device__ __forceinline__ void pd_eta_moments(int family, double eta, double sigma, double& m, double& v) {
  if (family == NUTS_GLM_NORMAL) pd_moments(NUTS_D_NORMAL, 0.0, eta, sigma, 0.0, &m, &v);
  else if (family == NUTS_GLM_BERNOULLI) pd_moments(NUTS_D_BERNOULLI_LOGIT, 0.0, eta, 0.0, 0.0, &m, &v);
  else pd_moments(NUTS_D_POISSON, 0.0, exp(eta), 0.0, 0.0, &m, &v);
}

// y: the held-out values in the node's evaluation order, or nullptr; lfact: factln(y) per row (Poisson with y), else nullptr
__global__ __launch_bounds__(LL_BLOCK) void k_pd_fold_eta(const double* __restrict__ eta, int nb, int64_t N, int family, const double* __restrict__ sc,
                                                          const double* __restrict__ y, const double* __restrict__ lfact, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
  double e[LL_B];
#pragma unroll
  for (int b = 0; b < LL_B; ++b) e[b] = b < nb ? eta[(int64_t)b * N + i] : 0.0;
  const double yi = y ? y[i] : 0.0, lf = (y && lfact) ? lfact[i] : 0.0;
  PDAcc a = pd_acc_load(acc, N, i);
#pragma unroll
  for (int b = 0; b < LL_B; ++b) {
    if (b >= nb) break;
    double m, v, lp = 0.0, rr, ds;
    pd_eta_moments(family, e[b], sc[4 * b + 1], m, v);
    if (y) { glm_row(family, e[b], yi, sc[4 * b + 1], sc[4 * b + 2], sc[4 * b + 3], lp, rr, ds); lp -= lf; }
    pd_fold(&a, m, v, lp, y != nullptr);
  }
  pd_acc_store(acc, N, i, a);
}

// the stage, in place, from eta to the conditional mean; var (nullptr: not wanted) gets the conditional variance
__global__ __launch_bounds__(LL_BLOCK) void k_pd_moments_eta(double* __restrict__ stage, int64_t N, int family, const double* __restrict__ sc,
                                                             double* __restrict__ var) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= N) return;
  double m, v;
  pd_eta_moments(family, stage[(int64_t)b * N + i], sc[4 * b + 1], m, v);
  stage[(int64_t)b * N + i] = m;
  if (var) var[(int64_t)b * N + i] = v;
}

// ---- b. element-wise factors ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LL_BLOCK) void k_pd_flags(ModelDev md, const double* __restrict__ q, int fi, int32_t* __restrict__ dead) {
  const Prog pg = prog_view(md, md.prog);
  const nuts_factor& f = pg.factors[fi];
  const int li = blockIdx.x * LL_BLOCK + threadIdx.x, b = blockIdx.y;
  if (li >= f.size) return;
  const QView qv = ll_view(q + (int64_t)b * md.n);
  double tv[NUTS_MAX_FACTOR_INSTR];
  ProgFwd o;
  prog_forward(pg, qv, f, li, -1, 0.0, tv, o);
  const DistOut r = dist_eval_v(f.dist, f.konst, o.a[0], o.a[1], o.a[2], o.a[3]);
  if (o.pdead || r.dead) dead[b] = 1;   // (every writer stores the same value)
}

// q: the batch's first position (positions md.n apart, or one position with nb = 1 where the factor reads per-position buffers)
__global__ __launch_bounds__(LL_BLOCK) void k_pd_fold_factor(ModelDev md, const double* __restrict__ q, int fi, int nb, const int32_t* __restrict__ dead,
                                                             int with_y, double* __restrict__ acc) {
  const Prog pg = prog_view(md, md.prog);
  const nuts_factor& f = pg.factors[fi];
  const int li = blockIdx.x * LL_BLOCK + threadIdx.x;
  if (li >= f.size) return;
  const int64_t N = f.size;
  PDAcc a = pd_acc_load(acc, N, li);
  double tv[NUTS_MAX_FACTOR_INSTR];
  for (int b = 0; b < nb; ++b) {
    const QView qv = ll_view(q + (int64_t)b * md.n);
    ProgFwd o;
    prog_forward(pg, qv, f, li, -1, 0.0, tv, o);
    double m, v, lp = 0.0;
    pd_moments(f.dist, f.konst, o.a[1], o.a[2], o.a[3], &m, &v);
    if (with_y) lp = dist_eval_v(f.dist, f.konst, o.a[0], o.a[1], o.a[2], o.a[3]).lp;
    if (dead[b]) { m = NAN; v = NAN; lp = -INFINITY; }
    pd_fold(&a, m, v, lp, with_y != 0);
  }
  pd_acc_store(acc, N, li, a);
}

__global__ __launch_bounds__(LL_BLOCK) void k_pd_moments_factor(ModelDev md, const double* __restrict__ q, int fi, double* __restrict__ mean,
                                                                double* __restrict__ var, int32_t* __restrict__ dead) {
  const Prog pg = prog_view(md, md.prog);
  const nuts_factor& f = pg.factors[fi];
  const int li = blockIdx.x * LL_BLOCK + threadIdx.x, b = blockIdx.y;
  if (li >= f.size) return;
  const QView qv = ll_view(q + (int64_t)b * md.n);
  double tv[NUTS_MAX_FACTOR_INSTR];
  ProgFwd o;
  prog_forward(pg, qv, f, li, -1, 0.0, tv, o);
  if (o.pdead || dist_eval_v(f.dist, f.konst, o.a[0], o.a[1], o.a[2], o.a[3]).dead) dead[b] = 1;   // (as k_pd_flags)
  double m, v;
  pd_moments(f.dist, f.konst, o.a[1], o.a[2], o.a[3], &m, &v);
  mean[(int64_t)b * f.size + li] = m;
  if (var) var[(int64_t)b * f.size + li] = v;
}

// ---- c. mixture node, marginal form --------------------------------------------------------------------------------------------
// lp of row value y under the K components in s_par = (mu, sigma, log w): the arithmetic of k_ll_mix
template <int KT>
__device__ __forceinline__ double pd_mix_lp(const double (*s_par)[MIX_MAXK], int K, double y) {
  double a[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    const int kk = min(k, K - 1);
    const double pm = s_par[0][kk], pis = 1.0 / s_par[1][kk];
    const double pk = k < K ? s_par[2][kk] - log(s_par[1][kk]) - 0.91893853320467274178 : -INFINITY;
    const double z = (y - pm) * pis;
    a[k] = fma(-0.5 * z, z, pk);
  }
  double amax = a[0];
#pragma unroll
  for (int k = 1; k < KT; ++k) amax = fmax(amax, a[k]);
  double se = 0.0;
#pragma unroll
  for (int k = 0; k < KT; ++k) se += exp(a[k] - amax);
  return amax + log(se);
}

// s_par[b] = (mu, sigma, log w, w) of draw b, by wave 0 (mix_params reduces over its first MIX_MAXK lanes)
__device__ __forceinline__ void pd_mix_load(const ModelDev& md, const double* __restrict__ q, int nb, double (*s_par)[4][MIX_MAXK]) {
  const MixDev& mx = md.mix;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid >> 6;
  if (w == 0) {
    for (int b = 0; b < nb; ++b) {
      const QView qv = ll_view(q + (int64_t)b * md.n);
      double mu, sg, lw, lse;
      mix_params(mx, qv, lane & (MIX_MAXK - 1), mu, sg, lw, lse);
      if (lane < mx.K) { s_par[b][0][lane] = mu; s_par[b][1][lane] = sg; s_par[b][2][lane] = lw; s_par[b][3][lane] = exp(lw); }
    }
  }
  __syncthreads();
}

template <int KT>
__global__ __launch_bounds__(MIX_BLOCK) void k_pd_fold_mix(ModelDev md, const double* __restrict__ q, int nb, int with_y, double* __restrict__ acc) {
  const MixDev& mx = md.mix;
  __shared__ double s_par[LL_B][4][MIX_MAXK];
  pd_mix_load(md, q, nb, s_par);
  const int64_t i = (int64_t)blockIdx.x * MIX_BLOCK + threadIdx.x;
  if (i >= mx.N) return;
  const double y = mx.y[i];
  PDAcc a = pd_acc_load(acc, mx.N, i);
  for (int b = 0; b < nb; ++b) {
    double m, v, lp = 0.0;
    pd_mixture(mx.K, s_par[b][0], s_par[b][1], s_par[b][3], &m, &v);
    if (with_y) lp = pd_mix_lp<KT>(s_par[b], mx.K, y);
    pd_fold(&a, m, v, lp, with_y != 0);
  }
  pd_acc_store(acc, mx.N, i, a);
}

__global__ __launch_bounds__(MIX_BLOCK) void k_pd_moments_mix(ModelDev md, const double* __restrict__ q, double* __restrict__ mean, double* __restrict__ var) {
  const MixDev& mx = md.mix;
  __shared__ double s_par[1][4][MIX_MAXK];
  const int b = blockIdx.y;
  pd_mix_load(md, q + (int64_t)b * md.n, 1, s_par);
  const int64_t i = (int64_t)blockIdx.x * MIX_BLOCK + threadIdx.x;
  if (i >= mx.N) return;
  double m, v;
  pd_mixture(mx.K, s_par[0][0], s_par[0][1], s_par[0][3], &m, &v);
  mean[(int64_t)b * mx.N + i] = m;
  if (var) var[(int64_t)b * mx.N + i] = v;
}
