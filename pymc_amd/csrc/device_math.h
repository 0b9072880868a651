// Device-side helpers: wavefront (64-lane) and workgroup reductions with a FIXED
// summation order (results are bit-reproducible run to run -- the reference
// promises "same seed => identical draws", tests/sampling/test_mcmc.py:80-109,
// so no floating-point atomics anywhere), plus the scalar special functions the
// log-densities need.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "scalar_math.h"   // softplus_d, sigmoid_d, logaddexp_d, digamma_d, trigamma_d, log1mexp_d

#define WAVE 64

// Wavefront sum on the DPP cross-lane network (VALU speed; `__shfl_*` would go through the LDS crossbar at ~100
// cycles per step).  Fixed association order:
//   rows of 16 lanes: shr 1, 2, 4, 8 (lane 15 of a row holds the row total), then row_bcast:15 folds row 0 into 1
//   and row 2 into 3, row_bcast:31 folds lanes 0-31 into row 3; lane 63 holds the total, which is read back as a
//   wave-uniform value (valid in EVERY lane).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move_d(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_move_d<0x111, 0xf>(v);  // row_shr:1
  v += dpp_move_d<0x112, 0xf>(v);  // row_shr:2
  v += dpp_move_d<0x114, 0xf>(v);  // row_shr:4
  v += dpp_move_d<0x118, 0xf>(v);  // row_shr:8
  v += dpp_move_d<0x142, 0xa>(v);  // row_bcast:15 -> rows 1 and 3
  v += dpp_move_d<0x143, 0xc>(v);  // row_bcast:31 -> rows 2 and 3
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, 63);
  hi = __builtin_amdgcn_readlane(hi, 63);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum_all(double v) { return wave_sum(v); }

// The same sum when only lanes 0 .. 7 can be non-zero (a group's D <= 8 z elements, rows_gb_kernel.h): after the first three
// steps lane 7 holds ((v7+v6)+(v5+v4))+((v3+v2)+(v1+v0)), and every later step of wave_sum only adds zeros to it -- the same
// number with half the dependent DPP steps.
__device__ __forceinline__ double wave_sum8(double v) {
  v += dpp_move_d<0x111, 0xf>(v);  // row_shr:1
  v += dpp_move_d<0x112, 0xf>(v);  // row_shr:2
  v += dpp_move_d<0x114, 0xf>(v);  // row_shr:4
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, 7);
  hi = __builtin_amdgcn_readlane(hi, 7);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    int o = __shfl_xor(v, off, WAVE);
    v = o < v ? o : v;
  }
  return v;
}

// Workgroup sum; `sm` must hold blockDim.x/64 doubles.  Result valid in thread 0
// (and broadcast through sm[0] after the trailing barrier when BCAST).
template <bool BCAST>
__device__ __forceinline__ double block_sum(double v, double* sm) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6, nw = (blockDim.x + WAVE - 1) >> 6;
  v = wave_sum(v);
  __syncthreads();  // protect sm from a previous use
  if (lane == 0) sm[w] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
    for (int i = 0; i < nw; ++i) r += sm[i];
    if (BCAST) sm[0] = r;
  }
  if (BCAST) {
    __syncthreads();
    r = sm[0];
  }
  return r;
}
