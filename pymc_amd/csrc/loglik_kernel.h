// Pointwise log-likelihood of observed factors and dense nodes at a BATCH of positions, and the streaming WAIC accumulators
// (include/nuts_mi355.h, nuts_model_loglik / nuts_waic_*): what `pm.compute_log_likelihood` and `az.waic` need from a finished trace.
//
// Every kernel evaluates at plain positions q[b][n] (the raveled UNCONSTRAINED draws, as the trace stores them: QView.composed = 0)
// and writes out[b][N].  Three rules:
//   * no atomics;
//   * the value of (draw, observation) never depends on how many draws share the launch: a draw is a column of the batch whose
//     arithmetic reads nothing of the other columns, and every kernel has ONE instantiation per layout whatever the batch holds
//     (unused columns are evaluated and not stored) -- alone, in a full batch or in a ragged last batch the bits are the same;
//   * the host uploads draws in blocks of LL_B, never the whole trace.
//
//   k_ll_factor   an element-wise factor: the interpreter's forward half (prog_forward + the density, model_dev.h), one thread per
//                 (draw, element).  A failed PARAMETER check kills the reference's whole factor at that draw: the kernel records
//                 the draw, k_ll_fill then writes -inf over its row.
//   k_ll_glm      the GLM node: the row layout of k_glm_rows (a row in the registers of `lpr` lanes, 16-byte coalesced loads, a
//                 contiguous row range per wave, the next iteration requested before the current one is evaluated) carrying B
//                 columns of beta' in registers -- X is read ONCE per batch, 8 N P / B + 8 N bytes per draw.  No backward half,
//                 no per-workgroup record, no reduce.
//   k_ll_rows     the hierarchical-logit rows: beta[b][g][d] = mu_d + sigma_d z_gd from a small pre-kernel, then a thread per
//                 (draw, row) reads its D columns from the model's resident copy of X in whichever layout it was built with.
//   k_ll_mix      the marginal Normal mixture: a thread per (draw, row), the row's logsumexp over K <= 16 components.
//   k_waic_fold   folds a [nb][N] block of values into the per-observation accumulators (m, r, mean, M2), draw by draw in draw order.
//   k_psis_fold   folds the same block into the PSIS-LOO state of each observation (psis.h): its K1 smallest values and the running
//                 log-sum of everything else; k_psis_finish fits and smooths each observation's tail once, at the end.
#pragma once
#include "kernels.h"
#include "mixture_kernel.h"
#include "psis.h"

#define LL_B 8          // draws per batch (the GLM kernel's register budget decides: see DESIGN.md, pointwise log-likelihood)
#define LL_BLOCK 256

__device__ __forceinline__ QView ll_view(const double* q) {
  QView qv;
  qv.q = q; qv.p = qv.g = qv.var = nullptr; qv.eps = qv.half = 0.0; qv.composed = 0;
  return qv;
}

// ---- a. element-wise factors ---------------------------------------------------------------------------------------------------
// q: the batch's first position; out: its first row (rows `size` apart); dead[b] = 1 when a parameter check of the factor failed at draw b
__global__ __launch_bounds__(LL_BLOCK) void k_ll_factor(ModelDev md, const double* __restrict__ q, int fi, double* __restrict__ out,
                                                        int32_t* __restrict__ dead) {
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
  out[(int64_t)b * f.size + li] = o.pdead ? -INFINITY : r.lp;
}

__global__ __launch_bounds__(LL_BLOCK) void k_ll_fill(double* __restrict__ out, int64_t size, const int32_t* __restrict__ dead) {
  const int64_t li = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (li < size && dead[b]) out[(int64_t)b * size + li] = -INFINITY;
}

// ---- b. GLM node ---------------------------------------------------------------------------------------------------------------
// Column b0 + blockIdx.x of the batch's parameters: Beta[b][Ppad] (exactly 0 beyond P: a row's last chunks read on into the next
// row) and sc[b] = {intercept, sigma, 1 / sigma, log sigma}.  A derived beta is read from the vector k_derive has just written.
__global__ __launch_bounds__(LL_BLOCK) void k_ll_glm_prep(ModelDev md, const double* __restrict__ q, int b0, double* __restrict__ Beta,
                                                          double* __restrict__ sc) {
  const GlmDev& gm = md.glm;
  const int b = b0 + blockIdx.x;
  const QView qv = ll_view(q + (int64_t)blockIdx.x * md.n);
  for (int col = threadIdx.x; col < gm.Ppad; col += LL_BLOCK)
    Beta[(int64_t)b * gm.Ppad + col] = col < gm.P ? (gm.beta_buf ? gm.beta_buf[col] : qv.at(gm.off_beta + col)) : 0.0;
  if (threadIdx.x == 0) {
    double icpt, sigma;
    glm_scalars(gm, qv, icpt, sigma);
    sc[4 * b + 0] = icpt; sc[4 * b + 1] = sigma; sc[4 * b + 2] = 1.0 / sigma;
    sc[4 * b + 3] = gm.family == NUTS_GLM_NORMAL ? log(sigma) : 0.0;
  }
}

// lf[i] = factln(y_i): the Poisson family's per-row constant (GlmDev.konst holds only the total), built once on first use
__global__ __launch_bounds__(LL_BLOCK) void k_ll_factln(const double* __restrict__ y, int64_t N, double* __restrict__ lf) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i < N) lf[i] = lgamma(y[i] + 1.0);
}

// The pass itself, shared with k_pp_glm (predictive_kernel.h): ETA = true stores the linear predictor instead of the row's value
template <int LPR, int CH, int B, bool ETA>
__device__ __forceinline__ void ll_glm_pass(const GlmDev& gm, const double* __restrict__ Beta, const double* __restrict__ sc, int nb,
                                            const double* __restrict__ lfact, double* __restrict__ out) {
  const int FAMILY = gm.family;
  constexpr int RPW = WAVE / LPR;
  constexpr int NW = GLM_BLOCK / WAVE;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid >> 6;
  const int sub = lane & (LPR - 1), grp = lane / LPR;
  const int Ppad = 2 * LPR * CH;
  const int64_t xstride = gm.xstride;
  // this wave's contiguous range of rows: the split of k_glm_rows
  const int64_t nwv = (int64_t)gridDim.x * NW, wv = (int64_t)blockIdx.x * NW + w;
  const int64_t per = ((gm.N + nwv - 1) / nwv + RPW - 1) / RPW * RPW;
  const int64_t r0 = wv * per, r1 = min(gm.N, r0 + per);
  const double* __restrict__ X = gm.X;
  double2 xn[CH];
  double yn;
  auto request = [&](int64_t r, double2 (&x)[CH], double& yv) {
    const int64_t row = min(r + grp, gm.N - 1);   // (rows past the range: valid addresses, masked below)
    const double2* p = reinterpret_cast<const double2*>(X + row * xstride) + sub;
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = p[c * LPR];
    yv = gm.y[row];
  };
  request(r0, xn, yn);
  // beta' of this lane's columns for the B draws, held in registers for the whole pass; the scalars are wave-uniform
  double2 bb[B][CH];
  double icpt[B], sigma[B], inv_sigma[B], log_sigma[B];
#pragma unroll
  for (int s = 0; s < B; ++s) {
    const double2* bp = reinterpret_cast<const double2*>(Beta + (int64_t)s * Ppad) + sub;
#pragma unroll
    for (int c = 0; c < CH; ++c) bb[s][c] = bp[c * LPR];
    icpt[s] = sc[4 * s + 0]; sigma[s] = sc[4 * s + 1]; inv_sigma[s] = sc[4 * s + 2]; log_sigma[s] = sc[4 * s + 3];
  }
  for (int64_t r = r0; r < r1; r += RPW) {
    double2 x[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = xn[c];
    const double y = yn;
    request(r + RPW, xn, yn);   // unconditional (past the end it re-reads clamped rows): in flight during the arithmetic
    const bool first = r + grp < r1 && sub == 0;   // one lane per row stores the row's values
    const int64_t row = r + grp;
    double lf = 0.0;
    if constexpr (!ETA) lf = lfact ? lfact[min(row, gm.N - 1)] : 0.0;   // Poisson: the row's own factln(y)
#pragma unroll
    for (int s = 0; s < B; ++s) {
      double part = 0.0;
#pragma unroll
      for (int c = 0; c < CH; ++c) { part = fma(x[c].x, bb[s][c].x, part); part = fma(x[c].y, bb[s][c].y, part); }
      const double eta = glm_group_sum<LPR>(part) + icpt[s];
      if constexpr (ETA) {
        if (first && s < nb) out[(int64_t)s * gm.N + row] = eta;
      } else {
        double lp, rr, ds;
        glm_row(FAMILY, eta, y, sigma[s], inv_sigma[s], log_sigma[s], lp, rr, ds);
        if (first && s < nb) out[(int64_t)s * gm.N + row] = lp - lf;
      }
    }
  }
}

template <int LPR, int CH, int B>
__global__ __launch_bounds__(GLM_BLOCK, 2) void k_ll_glm(GlmDev gm, const double* __restrict__ Beta, const double* __restrict__ sc, int nb,
                                                        const double* __restrict__ lfact, double* __restrict__ out) {
  ll_glm_pass<LPR, CH, B, false>(gm, Beta, sc, nb, lfact, out);
}

// ---- c. hierarchical-logit rows ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LL_BLOCK) void k_ll_rows_beta(ModelDev md, const double* __restrict__ q, double* __restrict__ beta) {
  const RowsDev& R = md.lg;
  const int64_t GD = (int64_t)R.G * R.D, i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= GD) return;
  const double* qb = q + (int64_t)b * md.n;
  const int d = (int)(i % R.D);
  const double s = qb[R.off_sigma + d], sg = R.sigma_tr == NUTS_TR_LOG ? exp(s) : s;
  beta[(int64_t)b * GD + i] = fma(sg, qb[R.off_z + i], qb[R.off_mu + d]);
}

// one thread per (draw, row in the spec's sorted order); LW: chunks per group of the per-group tile layout (build_rows_group)
// (the body is shared with k_pp_rows, predictive_kernel.h: ETA = true stores the linear predictor; YOBS = true the row's y instead)
template <bool ETA, bool YOBS>
__device__ __forceinline__ void ll_rows_body(const ModelDev& md, const double* __restrict__ beta, int span, int LW, double* __restrict__ out) {
  const RowsDev& R = md.lg;
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  const int b = blockIdx.y, D = R.D;
  if (i >= R.N) return;
  // the row's group: the last g with gptr[g] <= i (empty groups repeat a pointer)
  int lo = 0, hi = R.G;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (R.gptr[mid] <= i) lo = mid; else hi = mid; }
  const int g = lo;
  const double* bg = beta + ((int64_t)b * R.G + g) * D;
  double eta = 0.0, y;
  if (!R.ga) {   // span tiles [n_spans][D][span]
    const int64_t sp = i / span, rr = i % span;
    const double* x = R.Xt + sp * D * span + rr;
    for (int d = 0; d < D; ++d) eta = fma(x[(int64_t)d * span], bg[d], eta);
    y = (double)R.y[i];
  } else {       // per-group tiles [ga_dx][span], chunk (g, w) at ga_coff[g LW + w]; padded rows of a group's last tile belong to no i
    const int64_t r = i - R.gptr[g], t = r / span, rr = r % span;
    const int64_t T = R.ga_tile0[g + 1] - R.ga_tile0[g];
    int w = 0;
    while (w + 1 < LW && (int64_t)(w + 1) * T / LW <= t) ++w;
    const int DX = R.ga_dx;
    const int64_t base = R.ga_coff[(int64_t)g * LW + w] + (t - (int64_t)w * T / LW) * DX * span;
    const double* x = R.Xt + base + rr;
    if (DX == D - 1) eta = bg[0];   // the column of ones is not stored
    for (int d = D - DX; d < D; ++d) eta = fma(x[(int64_t)(d - (D - DX)) * span], bg[d], eta);
    y = (double)R.y[base / DX + rr];
  }
  if constexpr (YOBS) out[(int64_t)b * R.N + i] = y;
  else if constexpr (ETA) out[(int64_t)b * R.N + i] = eta;
  else {
    double lp, rj;
    logit_row(eta, y, lp, rj);
    out[(int64_t)b * R.N + i] = lp;
  }
}
__global__ __launch_bounds__(LL_BLOCK) void k_ll_rows(ModelDev md, const double* __restrict__ beta, int span, int LW, double* __restrict__ out) {
  ll_rows_body<false, false>(md, beta, span, LW, out);
}

// ---- d. mixture node, marginal form --------------------------------------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(MIX_BLOCK) void k_ll_mix(ModelDev md, const double* __restrict__ q, double* __restrict__ out) {
  const MixDev& mx = md.mix;
  const int b = blockIdx.y;
  const QView qv = ll_view(q + (int64_t)b * md.n);
  __shared__ double s_par[3][MIX_MAXK];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid >> 6, K = mx.K;
  if (w == 0) {
    double mu, sg, lw, lse;
    mix_params(mx, qv, lane & (MIX_MAXK - 1), mu, sg, lw, lse);
    if (lane < K) { s_par[0][lane] = mu; s_par[1][lane] = sg; s_par[2][lane] = lw; }
  }
  __syncthreads();
  double pm[KT], pis[KT], pk[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    const int kk = min(k, K - 1);
    pm[k] = s_par[0][kk];
    pis[k] = 1.0 / s_par[1][kk];
    pk[k] = k < K ? s_par[2][kk] - log(s_par[1][kk]) - 0.91893853320467274178 : -INFINITY;
  }
  const int64_t i = (int64_t)blockIdx.x * MIX_BLOCK + tid;
  if (i >= mx.N) return;
  const double y = mx.y[i];
  double a[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) { const double z = (y - pm[k]) * pis[k]; a[k] = fma(-0.5 * z, z, pk[k]); }
  double amax = a[0];
#pragma unroll
  for (int k = 1; k < KT; ++k) amax = fmax(amax, a[k]);
  double se = 0.0;
#pragma unroll
  for (int k = 0; k < KT; ++k) se += exp(a[k] - amax);
  out[(int64_t)b * mx.N + i] = amax + log(se);
}

// ---- e. WAIC accumulators ------------------------------------------------------------------------------------------------------
// acc = [4][N]: m (running maximum), r = sum exp(ll - m), mean, M2 (Welford).  One thread per observation folds the nb values of
// its column of the block in draw order; `count` draws were folded before.  ll = -inf leaves (m, r) as they are (it adds exp(-inf)
// = 0), never forms -inf - -inf.
__global__ __launch_bounds__(LL_BLOCK) void k_waic_fold(const double* __restrict__ ll, int nb, int64_t N, int64_t count, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
  double m = acc[i], r = acc[N + i], mean = acc[2 * N + i], M2 = acc[3 * N + i];
  for (int b = 0; b < nb; ++b) {
    const double v = ll[(int64_t)b * N + i];
    if (v > m) { r = (m == -INFINITY ? 0.0 : r * exp(m - v)) + 1.0; m = v; }
    else if (v > -INFINITY) r += exp(v - m);
    else if (v != v) { r = v; }   // (a NaN value is not hidden)
    const double k = (double)(count + b + 1);
    const double dl = v - mean;
    mean += dl / k;
    M2 = fma(dl, v - mean, M2);
  }
  acc[i] = m; acc[N + i] = r; acc[2 * N + i] = mean; acc[3 * N + i] = M2;
}
__global__ __launch_bounds__(LL_BLOCK) void k_waic_init(int64_t N, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
  acc[i] = -INFINITY; acc[N + i] = 0.0; acc[2 * N + i] = 0.0; acc[3 * N + i] = 0.0;
}

// ---- f. PSIS-LOO state (psis.h) ------------------------------------------------------------------------------------------------
// keep = [K1][N], rank-major (lane i and lane i + 1 touch neighbouring addresses), each column ascending in ll, +inf where empty;
// acc = [4][N]: (m, r) of ll as k_waic_fold keeps them (lppd), (m_rest, r_rest) of -ll over what is not kept.  One thread per
// observation folds its nb values in draw order.  A value not below the column's largest kept one (row K1 - 1: one coalesced
// read) goes straight to the running pair; a wave in which no lane inserts touches nothing else.  In a wave that inserts, the
// lanes walk the rank index j together from the bottom (psis_insert's loop runs while any lane still shifts), so every access to
// row j is one row of neighbouring addresses.
#define PSIS_FIN_BLOCK 64   // k_psis_finish: its candidates' work space, PSIS_WORK doubles per thread, is LDS
__global__ __launch_bounds__(LL_BLOCK) void k_psis_fold(const double* __restrict__ ll, int nb, int64_t N, int K1, double* __restrict__ keep,
                                                        double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
  double v[LL_B];
#pragma unroll
  for (int b = 0; b < LL_B; ++b) v[b] = b < nb ? ll[(int64_t)b * N + i] : 0.0;
  double m = acc[i], r = acc[N + i], mr = acc[2 * N + i], rr = acc[3 * N + i];
  double* col = keep + i;
  double thr = col[(int64_t)(K1 - 1) * N];
#pragma unroll
  for (int b = 0; b < LL_B; ++b) {
    if (b >= nb) break;
    const double x = v[b];
    if (x > m) { r = (m == -INFINITY ? 0.0 : r * exp(m - x)) + 1.0; m = x; }
    else if (x > -INFINITY) r += exp(x - m);
    else if (x != x) { r = x; }
    const bool ins = x < thr;
    if (!ins) psis_rest_fold(-x, mr, rr);
    if (__any(ins)) {
      if (ins) {
        const double out = psis_insert(col, N, K1, x);
        if (out != INFINITY) psis_rest_fold(-out, mr, rr);
        thr = col[(int64_t)(K1 - 1) * N];
      }
    }
  }
  acc[i] = m; acc[N + i] = r; acc[2 * N + i] = mr; acc[3 * N + i] = rr;
}

__global__ __launch_bounds__(LL_BLOCK) void k_psis_init(int64_t N, int K1, double* __restrict__ keep, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * LL_BLOCK + threadIdx.x;
  if (i >= N) return;
  for (int j = 0; j < K1; ++j) keep[(int64_t)j * N + i] = INFINITY;
  acc[i] = -INFINITY; acc[N + i] = 0.0; acc[2 * N + i] = -INFINITY; acc[3 * N + i] = 0.0;
}

// out = [3][N]: khat, elpd_loo_i, lppd_i = log r + m - log S.  The fit's candidates (b_j and the sums over the tail, m_est <= 61
// of each) are a column of LDS per thread, [PSIS_WORK][PSIS_FIN_BLOCK]: lane l at 8 l bytes of a row, no bank is asked twice.
__global__ __launch_bounds__(PSIS_FIN_BLOCK) void k_psis_finish(const double* __restrict__ keep, const double* __restrict__ acc, int64_t N,
                                                               int K1, int64_t S, double* __restrict__ out) {
  __shared__ double work[PSIS_WORK * PSIS_FIN_BLOCK];
  const int64_t i = (int64_t)blockIdx.x * PSIS_FIN_BLOCK + threadIdx.x;
  if (i >= N) return;
  const PsisOut o = psis_finish(keep + i, N, K1, acc[2 * N + i], acc[3 * N + i], S, work + threadIdx.x, PSIS_FIN_BLOCK);
  out[i] = o.khat;
  out[N + i] = o.elpd;
  out[2 * N + i] = log(acc[N + i]) + acc[i] - log((double)S);
}
