// Power-scaling sensitivity on the device (include/nuts_mi355.h, nuts_model_logdens_sum / nuts_psens_weights / nuts_psens; psens.h holds
// the definitions).
//
//   k_logdens_sum      the [nb][N] block of pointwise values nuts_model_loglik's kernels have just written, reduced per draw: workgroup
//   k_logdens_finish   (g, b) adds the elements g 256 + tid, + G 256, ... of draw b's row (a grid-stride loop on 64-bit indices), its
//                      lanes combine by butterfly, its waves in wave order; one workgroup per draw then adds the G partials in the
//                      same manner.  G follows from N alone (ld_groups), a draw's workgroups read nothing of the other draws: a
//                      draw's total does not depend on the batch, on the split of the draws over calls or on its company.  No atomics.
//                      A row holding -inf sums to -inf, a row holding NaN to NaN.
//   k_psens_weights    ONE WORKGROUP.  The column v = (1 - alpha) lc is sorted in LDS; its first K1 values are the column psis_fit
//                      expects, the log-sum of the others is one fixed-order sum over the SORTED values (so the fit does not depend on
//                      the order of the draws); thread 0 fits (psis.h, not restated), every thread then takes psis_weight of its draws.
//   k_psens            ONE WORKGROUP PER PARAMETER, fed by k_summary_transpose.  (key, draw number) pairs are sorted in LDS -- the
//                      bitonic network of k_summary with a payload and a lexicographic compare --; for each of the two alphas in turn
//                      the weights are gathered in sorted order, scanned inclusively (tiles of 256: a shuffle scan per wave, the waves
//                      and the carry in order) and the four sums of psens.h are taken for x and, walking the same data from the top,
//                      for -x.  Every sum in one fixed order: a thread adds the elements tid, tid + 256, ..., the lanes of a wave
//                      combine through a butterfly, the four waves in wave order.  A workgroup sees one parameter only: a
//                      parameter's row depends on its own draws and the two weight vectors, not on P, its neighbours or the blocks
//                      the host cuts P into.
//
// Ties.  Among equal keys only the cumulative weight at the END of the run enters the sums (bw = 0 inside it), but the order in
// which the run's weights are added rounds differently, and the draw number changes when the trace is permuted.  When a parameter
// has tied draws (one pass over neighbouring keys decides), the gathered weights are sorted once more as (key, weight) pairs: a run's
// weights are then added in ascending order of weight whatever the draws' numbers are, and the row is bitwise unchanged under a
// permutation of the draws together with their weights.  Without ties the second sort is skipped.
//
// LDS of k_psens at S = 8192 (160 KiB per CU): keys 64 KiB + scan 64 KiB + 16-bit draw numbers 16 KiB + the wave partials = 144.3 KiB;
// the two alphas SHARE the scan array, one after the other.  One workgroup per CU.  k_psens_weights: keys 64 KiB + the fit's work space.
#pragma once
#include <hip/hip_runtime.h>
#include "device_math.h"
#include "psens.h"
#include "psis.h"
#include "summary_kernel.h"

#define PS_BLOCK SUM_BLOCK
#define PS_MAX_S SUM_MAX_S
#define PS_NW (PS_BLOCK / WAVE)
#define LD_MAX_GROUPS 1024    // workgroups per draw of k_logdens_sum
#define LD_ITEMS 8            // elements per thread below which a draw gets fewer workgroups

// workgroups per draw: a function of N alone
static inline int ld_groups(int64_t N) {
  const int64_t g = (N + (int64_t)PS_BLOCK * LD_ITEMS - 1) / ((int64_t)PS_BLOCK * LD_ITEMS);
  return (int)(g < 1 ? 1 : (g > LD_MAX_GROUPS ? LD_MAX_GROUPS : g));
}

// the workgroup's sums of v[0 .. NS), the same bits in every thread; red: [PS_NW][NS] doubles of LDS
template <int NS>
__device__ __forceinline__ void ps_block_sums(double (&v)[NS], double* red) {
#pragma unroll
  for (int u = 0; u < NS; ++u) v[u] = sum_wave(v[u]);
  __syncthreads();   // (whoever still reads red[] is done)
  if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
    for (int u = 0; u < NS; ++u) red[(threadIdx.x / WAVE) * NS + u] = v[u];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    double t = red[u];
#pragma unroll
    for (int ww = 1; ww < PS_NW; ++ww) t += red[ww * NS + u];
    v[u] = t;
  }
}
__device__ __forceinline__ double ps_block_sum(double v, double* red) {
  double a[1] = {v};
  ps_block_sums<1>(a, red);
  return a[0];
}

// ---- a. per-draw totals ----------------------------------------------------------------------------------------------------------
// grid (G, nb); part[b * G + g]
__global__ __launch_bounds__(PS_BLOCK) void k_logdens_sum(const double* __restrict__ ll, int64_t N, double* __restrict__ part) {
  __shared__ double red[PS_NW];
  const double* __restrict__ row = ll + (int64_t)blockIdx.y * N;
  const int64_t step = (int64_t)gridDim.x * PS_BLOCK;
  double a = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * PS_BLOCK + threadIdx.x; i < N; i += step) a += row[i];
  a = ps_block_sum(a, red);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = a;
}
// grid (nb); out[b]
__global__ __launch_bounds__(PS_BLOCK) void k_logdens_finish(const double* __restrict__ part, int G, double* __restrict__ out) {
  __shared__ double red[PS_NW];
  const double* __restrict__ p = part + (int64_t)blockIdx.x * G;
  double a = 0.0;
  for (int g = threadIdx.x; g < G; g += PS_BLOCK) a += p[g];
  a = ps_block_sum(a, red);
  if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// ---- b. sorting pairs ------------------------------------------------------------------------------------------------------------
// ascending bitonic sort of (keys[i], pay[i]), i < npad (a power of two), by key, then by payload; a thread per compare-exchange
template <typename T>
__device__ __forceinline__ void ps_sort_pairs(double* keys, T* pay, int npad) {
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < npad / 2; t += PS_BLOCK) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const double a = keys[i], b = keys[i + j];
        const T pa = pay[i], pb = pay[i + j];
        const bool gt = a > b || (a == b && pa > pb);
        const bool lt = a < b || (a == b && pa < pb);
        if ((i & k) == 0 ? gt : lt) { keys[i] = b; keys[i + j] = a; pay[i] = pb; pay[i + j] = pa; }
      }
      __syncthreads();
    }
}

// ---- c. the weights of one alpha -------------------------------------------------------------------------------------------------
struct PsWeightLds {
  double keys[PS_MAX_S];
  double work[PSIS_WORK];
  double red[PS_NW * 2];
  PsisFit fit;
};

// lc: [S] on the device; w: [S]; khat: one double.  K1 = psis_tail_len(S, 1) + 1 <= S.
__global__ __launch_bounds__(PS_BLOCK) void k_psens_weights(const double* __restrict__ lc, int S, double alpha, int K1, double* __restrict__ w,
                                                           double* __restrict__ khat) {
  __shared__ PsWeightLds s;
  const int tid = threadIdx.x;
  int npad = 1;
  while (npad < S) npad <<= 1;
  double bad = 0.0;
  for (int j = tid; j < npad; j += PS_BLOCK) {
    double v = INFINITY;
    if (j < S) {
      const double c = lc[j];
      v = ps_column(alpha, c);
      bad += (ps_finite(c) && ps_finite(v)) ? 0.0 : 1.0;
      w[j] = v;   // the ROUNDED product, read back below: recomputed in place, -v - c would be contracted into one fma of the
    }             // unrounded product, and the draw at the cutoff would compare above the cutoff psis_fit took from the rounded key
    s.keys[j] = v;
  }
  if (ps_block_sum(bad, s.red) != 0.0) {   // (the same in every thread)
    for (int j = tid; j < S; j += PS_BLOCK) w[j] = NAN;
    if (tid == 0) *khat = NAN;
    return;
  }
  sum_sort(s.keys, npad);
  // everything beyond the kept column as one log-sum of -v: m_rest its largest term, r_rest = sum exp(-v - m_rest)
  const double m_rest = K1 < S ? -s.keys[K1] : -INFINITY;
  double r = 0.0;
  for (int j = K1 + tid; j < S; j += PS_BLOCK) r += exp(-s.keys[j] - m_rest);
  const double r_rest = ps_block_sum(r, s.red);
  if (tid == 0) s.fit = psis_fit(s.keys, 1, K1, m_rest, r_rest, (int64_t)S, s.work, 1);
  __syncthreads();
  const PsisFit f = s.fit;
  double acc = 0.0;
  for (int j = tid; j < S; j += PS_BLOCK) {
    const double wj = psis_weight(f, s.keys, 1, w[j]);   // (a thread reads back what it wrote itself)
    w[j] = wj;
    acc += wj;
  }
  const double total = ps_block_sum(acc, s.red);
  for (int j = tid; j < S; j += PS_BLOCK) w[j] = ps_normalise(w[j], total);   // (a thread reads back what it wrote itself)
  if (tid == 0) *khat = f.khat;
}

// ---- d. the distances of one parameter ---------------------------------------------------------------------------------------------
struct PsensLds {
  double keys[PS_MAX_S];      // the sorted draws
  double scan[PS_MAX_S];      // the gathered weights of the alpha in hand, then their inclusive scan
  uint16_t idx[PS_MAX_S];     // the draw number of each sorted key
  double red[PS_NW * 2 * PS_SUMS];
};

// scan[0 .. npad) <- its inclusive prefix sums, tile by tile
__device__ __forceinline__ void ps_scan(PsensLds& s, int npad) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  double carry = 0.0;
  __syncthreads();
  for (int base = 0; base < npad; base += PS_BLOCK) {
    double v = base + tid < npad ? s.scan[base + tid] : 0.0;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      const double u = __shfl_up(v, o, WAVE);
      if (lane >= o) v += u;
    }
    if (lane == WAVE - 1) s.red[wv] = v;
    __syncthreads();
    double off = carry;
    for (int ww = 0; ww < PS_NW; ++ww) {
      if (ww == wv) { if (base + tid < npad) s.scan[base + tid] = off + v; }
      off += s.red[ww];
    }
    carry = off;
    __syncthreads();   // (red[] is free again; the scan is visible after the last tile)
  }
}

// xt: [gridDim.x][S] rows of draws; w_lo, w_hi: [S] normalised weights; out[col * ldo + parameter]
__global__ __launch_bounds__(PS_BLOCK) void k_psens(const double* __restrict__ xt, int S, const double* __restrict__ w_lo,
                                                   const double* __restrict__ w_hi, double delta, double* __restrict__ out, int64_t ldo) {
  __shared__ PsensLds s;
  const int tid = threadIdx.x;
  const double* __restrict__ x = xt + (int64_t)blockIdx.x * S;
  int npad = 1;
  while (npad < S) npad <<= 1;
  double col[PS_COLS] = {NAN, NAN, NAN};

  double bad = 0.0;
  for (int j = tid; j < npad; j += PS_BLOCK) {
    const double v = j < S ? x[j] : INFINITY;
    s.keys[j] = v;
    s.idx[j] = (uint16_t)j;
    if (j < S) bad += ps_finite(v) ? 0.0 : 1.0;
  }
  const bool finite = ps_block_sum(bad, s.red) == 0.0;
  if (finite) {   // (the same in every thread)
    ps_sort_pairs<uint16_t>(s.keys, s.idx, npad);
    double ties = 0.0;
    for (int j = tid; j + 1 < S; j += PS_BLOCK) ties += s.keys[j] == s.keys[j + 1] ? 1.0 : 0.0;
    const bool tied = ps_block_sum(ties, s.red) != 0.0;
    for (int a = 0; a < 2; ++a) {
      const double* __restrict__ w = a == 0 ? w_lo : w_hi;
      __syncthreads();   // (the sums of the alpha before have read scan[])
      for (int j = tid; j < npad; j += PS_BLOCK) s.scan[j] = j < S ? w[s.idx[j]] : 0.0;
      if (tied) ps_sort_pairs<double>(s.keys, s.scan, npad);   // (equal keys change places only: idx[] still names a draw of each run)
      ps_scan(s, npad);
      const double total = s.scan[S - 1];
      double acc[2 * PS_SUMS];
#pragma unroll
      for (int u = 0; u < 2 * PS_SUMS; ++u) acc[u] = 0.0;
      for (int j = tid; j < S - 1; j += PS_BLOCK) {
        const double P = (double)(j + 1) / (double)S;
        ps_term(s.keys[j + 1] - s.keys[j], P, s.scan[j], acc);
        const int k = S - 2 - j;   // element j of -x sorted: the same data from the top
        double Qr = total - s.scan[k];
        if (Qr < 0.0) Qr = 0.0;    // (the tiled scan is not monotone to the last bit)
        ps_term(s.keys[k + 1] - s.keys[k], P, Qr, acc + PS_SUMS);
      }
      ps_block_sums<2 * PS_SUMS>(acc, s.red);
      col[a] = ps_cjs(ps_distance(acc), ps_distance(acc + PS_SUMS));
    }
    col[PS_SENS] = ps_sensitivity(col[PS_CJS_LO], col[PS_CJS_HI], delta);
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < PS_COLS; ++k) out[(int64_t)k * ldo + blockIdx.x] = col[k];
  }
}
