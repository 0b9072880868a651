// Model comparison on the device (compare.h holds the arithmetic and the solver).  State: e[K][N] (the pointwise elpd
// of every model, observation fastest) and p[K][N] (the shifted stacking terms).  Every kernel is templated on K = 2 .. CMP_MAXK so
// that the accumulators are registers.  No atomics: a thread adds its observations in index order, the lanes of a wave are combined
// by a fixed butterfly, the waves of a workgroup in wave order into the slot part[workgroup][accumulator], and k_cmp_reduce adds the
// slots of an accumulator in one fixed order -- a result depends on the number of workgroups (the option NUTS_COMPARE_WGS) and on
// nothing else.
//
//   k_cmp_scatter      row k from the staged host vector, through the caller's permutation if there is one
//   k_cmp_moments      PASS 0: sum_i e_ik;  PASS 1: sum_i (e_ik - mean_k)^2 and sum_i ((e_i,best - e_ik) - dmean_k)^2 -- two passes, as np.var
//   k_cmp_terms        p_ik = exp(e_ik - m_i) and sum_i m_i, once per set of rows
//   k_cmp_stack_pass   the hot path of stacking: streams p (8 K N bytes) and accumulates the CMP_NACC(K) sums of compare.h at w
//   k_cmp_bb           the Bayesian bootstrap.  One WAVE per workgroup; a workgroup owns a contiguous range of slabs of
//                      CMP_BB_SLAB = 64 x CMP_BB_R observations.  Per slab a lane holds the e_ik of its CMP_BB_R observations in
//                      registers and loops over the launch's replicate PAIRS: one Philox block per observation gives g of replicates
//                      2 j and 2 j + 1.  After the butterfly lane 0 adds the pair's 2 (K + 1) sums (sum g, sum g e_.k) to the
//                      workgroup's own slots part[workgroup][replicate][K + 1] (written at its first slab, added to at the others).
//                      The order in which a replicate's observations are added is (register, lane butterfly, slab, workgroup): it
//                      does not depend on the number of replicates or on how they are cut into launches.
#pragma once
#include "compare.h"
#include "device_math.h"

#define CMP_BLOCK 256
#define CMP_BB_R 4
#define CMP_BB_SLAB (WAVE * CMP_BB_R)
#define CMP_BB_CHUNK 256   // replicates per launch (bounds part at workgroups x 256 x (K + 1) doubles)

struct CmpVec { double v[CMP_MAXK]; };

// the NA sums of the workgroup into out[0 .. NA)
template <int NA>
__device__ __forceinline__ void cmp_block_sum(double (&a)[NA], double* __restrict__ out) {
  __shared__ double s_w[CMP_BLOCK / WAVE][NA];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    double v = a[j];
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o, WAVE);
    if (lane == 0) s_w[w][j] = v;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < NA; j += CMP_BLOCK) {
    double s = s_w[0][j];
#pragma unroll
    for (int ww = 1; ww < CMP_BLOCK / WAVE; ++ww) s += s_w[ww][j];
    out[j] = s;
  }
}

__global__ __launch_bounds__(CMP_BLOCK) void k_cmp_scatter(const double* __restrict__ src, const int64_t* __restrict__ order, int64_t N,
                                                           double* __restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * CMP_BLOCK + threadIdx.x;
  if (j >= N) return;
  dst[order ? order[j] : j] = src[j];   // (order is a permutation of 0 .. N - 1: nuts_compare_set checked it)
}

template <int K, int PASS>
__global__ __launch_bounds__(CMP_BLOCK) void k_cmp_moments(const double* __restrict__ e, int64_t N, CmpVec mean, CmpVec dmean, int best,
                                                           double* __restrict__ part) {
  constexpr int NA = PASS == 0 ? K : 2 * K;
  double a[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) a[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * CMP_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * CMP_BLOCK) {
    double x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = e[(int64_t)k * N + i];
    if (PASS == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) a[k] += x[k];
    } else {
      const double xb = e[(int64_t)best * N + i];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double c = x[k] - mean.v[k], d = (xb - x[k]) - dmean.v[k];
        a[k] = fma(c, c, a[k]);
        a[K + k] = fma(d, d, a[K + k]);
      }
    }
  }
  cmp_block_sum<NA>(a, part + (int64_t)blockIdx.x * NA);
}

template <int K>
__global__ __launch_bounds__(CMP_BLOCK) void k_cmp_terms(const double* __restrict__ e, int64_t N, double* __restrict__ p, double* __restrict__ part) {
  double a[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * CMP_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * CMP_BLOCK) {
    double x[K], t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = e[(int64_t)k * N + i];
    a[0] += cmp_terms<K>(x, t);
#pragma unroll
    for (int k = 0; k < K; ++k) p[(int64_t)k * N + i] = t[k];
  }
  cmp_block_sum<1>(a, part + blockIdx.x);
}

template <int K>
__global__ __launch_bounds__(CMP_BLOCK) void k_cmp_stack_pass(const double* __restrict__ p, int64_t N, CmpVec wv, double* __restrict__ part) {
  constexpr int NA = CMP_NACC(K);
  double a[NA], w[K];
#pragma unroll
  for (int j = 0; j < NA; ++j) a[j] = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = wv.v[k];
  for (int64_t i = (int64_t)blockIdx.x * CMP_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * CMP_BLOCK) {
    double x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = p[(int64_t)k * N + i];
    cmp_pass_add<K>(x, w, a);
  }
  cmp_block_sum<NA>(a, part + (int64_t)blockIdx.x * NA);
}

// One workgroup per accumulator a < na: thread t adds the slots of the workgroups t, t + CMP_BLOCK, ... in that order, then the
// threads' totals are combined as cmp_block_sum combines lanes and waves.
__global__ __launch_bounds__(CMP_BLOCK) void k_cmp_reduce(const double* __restrict__ part, int64_t nwg, int64_t na, double* __restrict__ out) {
  double a[1] = {0.0};
  for (int64_t g = threadIdx.x; g < nwg; g += CMP_BLOCK) a[0] += part[g * na + blockIdx.x];
  cmp_block_sum<1>(a, out + blockIdx.x);
}

// replicates 2 pair0 .. 2 (pair0 + npairs) - 1; part = [gridDim.x][2 npairs][K + 1]; gridDim.x <= nslab
template <int K>
__global__ __launch_bounds__(WAVE) void k_cmp_bb(const double* __restrict__ e, int64_t N, int64_t nslab, PPKey key, uint32_t pair0, int npairs,
                                                 double* __restrict__ part) {
  const int lane = threadIdx.x;
  const int64_t s_lo = (int64_t)blockIdx.x * nslab / gridDim.x, s_hi = ((int64_t)blockIdx.x + 1) * nslab / gridDim.x;
  double* mine = part + (int64_t)blockIdx.x * 2 * npairs * (K + 1);
  if (s_lo >= s_hi) {   // (not reached while gridDim.x <= nslab; the slots are defined all the same)
    for (int j = lane; j < 2 * npairs * (K + 1); j += WAVE) mine[j] = 0.0;
    return;
  }
  for (int64_t slab = s_lo; slab < s_hi; ++slab) {
    double x[CMP_BB_R][K];
    int64_t idx[CMP_BB_R];
#pragma unroll
    for (int r = 0; r < CMP_BB_R; ++r) {
      idx[r] = slab * CMP_BB_SLAB + r * WAVE + lane;
#pragma unroll
      for (int k = 0; k < K; ++k) x[r][k] = idx[r] < N ? e[(int64_t)k * N + idx[r]] : 0.0;
    }
    for (int jp = 0; jp < npairs; ++jp) {
      double a0[K + 1], a1[K + 1];
#pragma unroll
      for (int j = 0; j <= K; ++j) { a0[j] = 0.0; a1[j] = 0.0; }
#pragma unroll
      for (int r = 0; r < CMP_BB_R; ++r) {
        double g0, g1;
        cmp_g_pair(key, idx[r], pair0 + (uint32_t)jp, g0, g1);
        if (idx[r] >= N) { g0 = 0.0; g1 = 0.0; }
        a0[0] += g0; a1[0] += g1;
#pragma unroll
        for (int k = 0; k < K; ++k) { a0[1 + k] = fma(g0, x[r][k], a0[1 + k]); a1[1 + k] = fma(g1, x[r][k], a1[1 + k]); }
      }
#pragma unroll
      for (int j = 0; j <= K; ++j) {
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) { a0[j] += __shfl_xor(a0[j], o, WAVE); a1[j] += __shfl_xor(a1[j], o, WAVE); }
      }
      if (lane == 0) {
        double* q = mine + (int64_t)2 * jp * (K + 1);
        if (slab == s_lo) {
#pragma unroll
          for (int j = 0; j <= K; ++j) { q[j] = a0[j]; q[K + 1 + j] = a1[j]; }
        } else {
#pragma unroll
          for (int j = 0; j <= K; ++j) { q[j] += a0[j]; q[K + 1 + j] += a1[j]; }
        }
      }
    }
  }
}
