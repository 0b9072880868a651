// The convergence summary of a trace on the device (include/nuts_mi355.h, nuts_summary): mean, sd, HDI, MCSE of the
// mean and of the sd, bulk and tail ESS and split R-hat of every parameter, as summary.h defines them.
//
//   k_summary_transpose   [C N][B] (parameters fastest, as a trace is stored) -> [B][C N]: one parameter's draws become one contiguous row
//   k_summary             ONE WORKGROUP PER PARAMETER.  The S = C N draws are sorted in LDS (a bitonic network over the next power of
//                         two, padded with +inf); the sorted keys give the HDI, the pooled 5 % / 95 % quantiles, the median and --
//                         through a lower and an upper bound search of every draw -- the average ranks, so no (key, position) pairs
//                         are carried.  A second sort of |x - median| gives the folded ranks.  Each of the five arrays behind an ESS (z,
//                         x, (x - mean)^2 and the two tail indicators, all in split-chain layout) is laid into a second LDS array, centred
//                         per chain, and its autocovariances are formed as direct lagged products, SUM_LAGS lags per pass and only as far
//                         as the Geyer scan (summary.h) asks: two workgroup barriers per SUM_LAGS lags, no reduction per scan step.
//
// Every sum is taken in one fixed order -- a thread adds the elements tid, tid + 256, ... in that order, the lanes of a wave combine
// through a butterfly, the four waves in wave order -- and a workgroup sees one parameter only: a parameter's row of the result does
// not depend on P, on its neighbours or on the blocks the host cuts P into.  No atomics.
//
// LDS: two arrays of SUM_MAX_S doubles (128 KiB) and the wave partials; one workgroup per CU.
#pragma once
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "summary.h"

#define SUM_BLOCK 256
#define SUM_MAX_S 8192   // draws of one parameter (chains x draws); nuts_summary_max_draws()
#define SUM_LAGS 8
#define SUM_TILE 32

__global__ __launch_bounds__(SUM_BLOCK) void k_summary_transpose(const double* __restrict__ in, int64_t R, int64_t B, double* __restrict__ out) {
  __shared__ double tile[SUM_TILE][SUM_TILE + 1];
  const int tx = threadIdx.x & (SUM_TILE - 1), ty = threadIdx.x / SUM_TILE;
  const int64_t r0 = (int64_t)blockIdx.y * SUM_TILE, b0 = (int64_t)blockIdx.x * SUM_TILE;
  for (int k = ty; k < SUM_TILE; k += SUM_BLOCK / SUM_TILE)
    if (r0 + k < R && b0 + tx < B) tile[k][tx] = in[(r0 + k) * B + b0 + tx];
  __syncthreads();
  for (int k = ty; k < SUM_TILE; k += SUM_BLOCK / SUM_TILE)
    if (b0 + k < B && r0 + tx < R) out[(b0 + k) * R + r0 + tx] = tile[tx][k];
}

struct SumLds {
  double keys[SUM_MAX_S];   // the sort; between sorts: the chain means of the array in w
  double w[SUM_MAX_S];      // the array an ESS / R-hat is being taken of, split-chain layout [2 C][N / 2]
  double red[SUM_BLOCK / WAVE][SUM_LAGS];
};

__device__ __forceinline__ double sum_wave(double v) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}
// the workgroup's sum of v, the same bits in every thread
__device__ __forceinline__ double sum_block(SumLds& s, double v) {
  v = sum_wave(v);
  __syncthreads();   // (whoever still reads red[] is done)
  if ((threadIdx.x & (WAVE - 1)) == 0) s.red[threadIdx.x / WAVE][0] = v;
  __syncthreads();
  double t = s.red[0][0];
#pragma unroll
  for (int ww = 1; ww < SUM_BLOCK / WAVE; ++ww) t += s.red[ww][0];
  return t;
}

// ascending bitonic sort of keys[0 .. npad), npad a power of two; a thread per compare-exchange
__device__ __forceinline__ void sum_sort(double* keys, int npad) {
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < npad / 2; t += SUM_BLOCK) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const double a = keys[i], b = keys[i + j];
        if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[i + j] = a; }
      }
      __syncthreads();
    }
}

// element j of split(x): chains 0 .. C-1 are the first halves, C .. 2C-1 the second halves (stats._split)
__device__ __forceinline__ double sum_split(const double* __restrict__ x, int C, int N, int h, int j) {
  const int cs = j / h, i = j - cs * h;
  return cs < C ? x[cs * N + i] : x[(cs - C) * N + (N - h) + i];
}

// the z-score of v's average rank among the sorted keys[0 .. n)
__device__ __forceinline__ double sum_rank_z(const double* keys, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (keys[m] < v) lo = m + 1; else hi = m; }
  int lo2 = lo, hi2 = n;
  while (lo2 < hi2) { const int m = (lo2 + hi2) >> 1; if (keys[m] <= v) lo2 = m + 1; else hi2 = m; }
  return sm_rank_z(0.5 * (double)(lo + lo2 + 1), n);
}

// Centre every chain of w[nch][n] on its own mean (a wave per chain; the means go to keys[0 .. nch)); ss = the sum of squares of the
// centred array, var_means = the variance (ddof = 1) of the chain means.
__device__ __forceinline__ void sum_centre(SumLds& s, int nch, int n, double& ss, double& var_means) {
  const int lane = threadIdx.x & (WAVE - 1);
  __syncthreads();
  for (int c = threadIdx.x / WAVE; c < nch; c += SUM_BLOCK / WAVE) {
    double* wc = s.w + c * n;
    double a = 0.0;
    for (int i = lane; i < n; i += WAVE) a += wc[i];
    const double m = sum_wave(a) / (double)n;
    if (lane == 0) s.keys[c] = m;
    for (int i = lane; i < n; i += WAVE) wc[i] -= m;
  }
  __syncthreads();
  double a = 0.0, b = 0.0;
  for (int j = threadIdx.x; j < nch * n; j += SUM_BLOCK) a += s.w[j] * s.w[j];
  ss = sum_block(s, a);
  for (int c = threadIdx.x; c < nch; c += SUM_BLOCK) b += s.keys[c];
  const double gm = sum_block(s, b) / (double)nch;
  b = 0.0;
  for (int c = threadIdx.x; c < nch; c += SUM_BLOCK) b += (s.keys[c] - gm) * (s.keys[c] - gm);
  var_means = sum_block(s, b) / (double)(nch - 1);
}

// red[.][u] <- the waves' partial sums of w[c][i] w[c][i + t0 + u] over all chains c and i < n - t0 - u, u < SUM_LAGS
__device__ __forceinline__ void sum_lags(SumLds& s, int nch, int n, int t0) {
  double acc[SUM_LAGS];
#pragma unroll
  for (int u = 0; u < SUM_LAGS; ++u) acc[u] = 0.0;
  int i = threadIdx.x % n;
  for (int j = threadIdx.x; j < nch * n; j += SUM_BLOCK) {
    const double a = s.w[j];
#pragma unroll
    for (int u = 0; u < SUM_LAGS; ++u)
      if (i + t0 + u < n) acc[u] += a * s.w[j + t0 + u];
    i = (i + SUM_BLOCK) % n;
  }
#pragma unroll
  for (int u = 0; u < SUM_LAGS; ++u) acc[u] = sum_wave(acc[u]);
  __syncthreads();   // (every thread has read the lags of the block before)
  if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
    for (int u = 0; u < SUM_LAGS; ++u) s.red[threadIdx.x / WAVE][u] = acc[u];
  }
  __syncthreads();
}

// ESS of the array in w (summary.h, sm_ess); leaves w centred.  rhat != nullptr: its split R-hat as well.
__device__ __forceinline__ double sum_ess(SumLds& s, int nch, int n, double* rhat) {
  double ss, vm;
  sum_centre(s, nch, n, ss, vm);
  if (rhat) *rhat = sm_rhat(n, ss / (double)(n - 1) / (double)nch, (double)n * vm);
  const double tot = (double)n * (double)nch;
  int have = 0;   // the block of lags red[] holds starts here (0: none)
  return sm_ess(nch, n, ss / tot, vm, [&](int64_t t) {
    const int t0 = (((int)t - 1) / SUM_LAGS) * SUM_LAGS + 1;
    if (t0 != have) { sum_lags(s, nch, n, t0); have = t0; }
    double v = s.red[0][(int)t - t0];
#pragma unroll
    for (int ww = 1; ww < SUM_BLOCK / WAVE; ++ww) v += s.red[ww][(int)t - t0];
    return v / tot;
  });
}

// x: [gridDim.x][S] rows of S = C N draws, chain-major; out[col * ldo + parameter]
__global__ __launch_bounds__(SUM_BLOCK) void k_summary(const double* __restrict__ xt, int C, int N, double hdi_prob, double* __restrict__ out, int64_t ldo) {
  __shared__ SumLds s;
  const int tid = threadIdx.x, S = C * N;
  const double* __restrict__ x = xt + (int64_t)blockIdx.x * S;
  double col[SM_COLS];
#pragma unroll
  for (int k = 0; k < SM_COLS; ++k) col[k] = NAN;
  int npad = 1;
  while (npad < S) npad <<= 1;

  // ---- all S draws: finite?, mean, the sums of d = (x - mean)^2 and d^2, the sorted keys ----
  double a = 0.0, b = 0.0;
  for (int j = tid; j < npad; j += SUM_BLOCK) {
    const double v = j < S ? x[j] : INFINITY;
    s.keys[j] = v;
    if (j < S) { a += v; b += (v - v == 0.0) ? 0.0 : 1.0; }
  }
  const bool finite = sum_block(s, b) == 0.0;
  const double mean = sum_block(s, a) / (double)S;
  if (finite) {   // (the same in every thread)
    a = 0.0; b = 0.0;
    for (int j = tid; j < S; j += SUM_BLOCK) { const double d = (x[j] - mean) * (x[j] - mean); a += d; b += d * d; }
    const double sum_d = sum_block(s, a), sum_d2 = sum_block(s, b);
    col[SM_MEAN] = mean;
    col[SM_SD] = sm_sd(sum_d, S);
    sum_sort(s.keys, npad);
    const int64_t k = sm_hdi_k(hdi_prob, S);
    if (S - k >= 1) {
      double bw; int64_t bi;
      sm_hdi_scan(s.keys, S, k, tid, SUM_BLOCK, bw, bi);
#pragma unroll
      for (int o = 1; o < WAVE; o <<= 1) {
        const double ow = __shfl_xor(bw, o, WAVE);
        const int64_t oi = __shfl_xor((int)bi, o, WAVE);
        if (sm_hdi_better(ow, oi, bw, bi)) { bw = ow; bi = oi; }
      }
      __syncthreads();
      if ((tid & (WAVE - 1)) == 0) { s.red[tid / WAVE][0] = bw; s.red[tid / WAVE][1] = (double)bi; }
      __syncthreads();
      bw = s.red[0][0]; bi = (int64_t)s.red[0][1];
      for (int ww = 1; ww < SUM_BLOCK / WAVE; ++ww)
        if (sm_hdi_better(s.red[ww][0], (int64_t)s.red[ww][1], bw, bi)) { bw = s.red[ww][0]; bi = (int64_t)s.red[ww][1]; }
      col[SM_HDI_LO] = s.keys[bi];
      col[SM_HDI_HI] = s.keys[bi + k];
    }
    const double q05 = sm_quantile(s.keys, S, 0.05), q95 = sm_quantile(s.keys, S, 0.95);

    // ---- split chains: [2 C][h]; with N odd the middle draw of every chain leaves the sorted set ----
    const int h = N / 2, nch = 2 * C, S2 = nch * h;
    if (h >= 1) {
      if (N & 1) {
        __syncthreads();
        for (int j = tid; j < npad; j += SUM_BLOCK) s.keys[j] = j < S2 ? sum_split(x, C, N, h, j) : INFINITY;
        sum_sort(s.keys, npad);
      }
      const double median = (s.keys[S2 / 2 - 1] + s.keys[S2 / 2]) / 2.0;
      for (int j = tid; j < S2; j += SUM_BLOCK) s.w[j] = sum_rank_z(s.keys, S2, sum_split(x, C, N, h, j));
      double rh_bulk, rh_fold;
      col[SM_ESS_BULK] = sum_ess(s, nch, h, &rh_bulk);   // (its barrier comes before keys[] is overwritten)

      __syncthreads();
      for (int j = tid; j < npad; j += SUM_BLOCK) s.keys[j] = j < S2 ? fabs(sum_split(x, C, N, h, j) - median) : INFINITY;
      sum_sort(s.keys, npad);
      for (int j = tid; j < S2; j += SUM_BLOCK) s.w[j] = sum_rank_z(s.keys, S2, fabs(sum_split(x, C, N, h, j) - median));
      double ss, vm;
      sum_centre(s, nch, h, ss, vm);
      rh_fold = sm_rhat(h, ss / (double)(h - 1) / (double)nch, (double)h * vm);
      col[SM_R_HAT] = sm_pymax(rh_bulk, rh_fold);

      __syncthreads();
      for (int j = tid; j < S2; j += SUM_BLOCK) s.w[j] = sum_split(x, C, N, h, j);
      col[SM_MCSE_MEAN] = col[SM_SD] / sqrt(sum_ess(s, nch, h, nullptr));
      __syncthreads();
      for (int j = tid; j < S2; j += SUM_BLOCK) { const double v = sum_split(x, C, N, h, j) - mean; s.w[j] = v * v; }
      col[SM_MCSE_SD] = sm_mcse_sd(sum_d, sum_d2, S, sum_ess(s, nch, h, nullptr));
      __syncthreads();
      for (int j = tid; j < S2; j += SUM_BLOCK) s.w[j] = sum_split(x, C, N, h, j) <= q05 ? 1.0 : 0.0;
      const double e05 = sum_ess(s, nch, h, nullptr);
      __syncthreads();
      for (int j = tid; j < S2; j += SUM_BLOCK) s.w[j] = sum_split(x, C, N, h, j) <= q95 ? 1.0 : 0.0;
      col[SM_ESS_TAIL] = sm_pymin(e05, sum_ess(s, nch, h, nullptr));
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < SM_COLS; ++k) out[(int64_t)k * ldo + blockIdx.x] = col[k];
  }
}
