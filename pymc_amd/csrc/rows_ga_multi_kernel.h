// Lockstep chains of ONE hierarchical-logit model on the group-aligned row pass (the benchmark's model, BASELINE configs[1]: eight
// chains; the reference runs chains as independent processes, pymc/sampling/mcmc.py:1385-1500, sampling/parallel.py:477-589, and
// vmaps them on an accelerator, sampling/jax.py:341-348).
//
// `k_rows_ga` (rows_ga_kernel.h) is bound by the bytes of X: 99.6 % of what a leapfrog reads is the design matrix, which every
// chain of a rank reads identically.  `k_rows_ga_multi<NC, OCC, DX>` is the same launch for NC chains that stand at a tree leaf at
// the same time (engine.hip, the chain group: each chain's host thread deposits its launch, the last one to arrive submits them
// together): workgroup g streams the tiles of group g ONCE and evaluates every row under NC coefficient vectors (beta_g of each
// chain in scalar registers, NC sets of gradient accumulators), then finishes the group's D z elements of every chain -- second
// kick, v', merge dot products, the group's record, the ticket on the chain's own arrival counters: that IS the single-chain
// kernel's tail (ga_tail_wave, ga_block_partial of rows_ga_kernel.h on the chain's buffers), one wave per chain.  Workgroups 0 .. GAM_MAXC-1 carry the control work each chain folds into its launch (a
// chain's always in workgroup `slot`, i.e. on the same XCD).
//
// A chain's numbers do not depend on its company: every fma of a row, every wave sum (the exchange tree of mvn_multi_kernel.h
// reproduces `wave_sum`'s association order), every record and block partial is formed from the chain's own operands by the
// single-chain kernel's code, so a chain in a group is BITWISE the chain run alone (tests/test_gpu_chain_group.py).
//
// Chains keep their own arena, control block, uniform stream, status words, records, block partials, tickets and local parts
// (`ga_part`, `ga_bpart`, `ga_ticket`, `def_loc` of the chain's own model handle): nothing is shared but the read-only node data
// (X, y, the closed-form priors) and the in-order stream the group submits to.
//
// The pass is then bound by the vector pipe, not by HBM: ~73 fp64 operations per row and chain (logit_row) against 57 bytes per
// row -- one chain needs ~15 us of arithmetic for a 45 us stream, four chains are arithmetic-bound.
#pragma once
#include "mvn_multi_kernel.h"   // (wave_sum_many)

#define GAM_MAXC 8   // control workgroups of a launch = places in a rows group (round 6: eight, rows_gal_kernel.h; THIS kernel carries at most GAM_MAXNC chains)
#define GAM_MAXNC 4

struct GaLeafArgs {   // one chain's arguments of k_rows_ga (GaArgs without the model)
  ArenaDev A;
  EvalIO io, cio;
  double Emax;
  HostStatus* st;
  double* ga_part;       // [G][PART_STRIDE]           this chain's per-group records
  double* ga_bpart;      // [2][ga_nrec][PART_STRIDE]  its block partials, double-buffered by ITS launch parity
  unsigned* ga_ticket;   // [ga_nblk]                  its arrival counters
  double* def_loc;       // [2][MAX_DEFERRED][4]       local parts of its hyper-parameter elements
  int j, fold, par, d, max_depth, cj, cd, cseq;
  int slot, pad;         // the chain's place in its group: its control work always runs in workgroup `slot`
};

template <int NC, bool SH = false>
struct GaMultiArgs {
  GaLeafArgs c[NC];
  int rev, pad;          // traversal order of a wave's two half-ranges in THIS launch (the result does not depend on it)
};
// SH (edge pairing; NC = 2): c[0] is the chain at a tree leaf, c[1] the SHADOW leaf -- the next leapfrog of the
// trajectory's other end, a plain leapfrog chain (MODE_SIMPLE: no tree work, no control work) on buffers of its own: a two-slot
// arena view, records, block partials, tickets, local parts.  `c[1].pad` bit 0: the shadow sequence starts here, its source
// state is the other end's edge state in c[0]'s arena (with GA_FOLD_SRC: that state is the leaf of c[0]'s previous launch, so
// mu' / sigma' come from c[0]'s block partials, as for a leaf of the chain itself).  The shadow leaf's finished wave sums go to
// `ring`, this leaf's ring entry ([G][GA_MAXW][2][D + 1], rows_ga_kernel.h: k_rows_ga_replay picks them up).
#define GAM_SH_FIRST 1
template <int NC>
struct GaMultiArgs<NC, true> {
  GaLeafArgs c[NC];
  int rev, pad;
  double* ring;
};

__device__ __forceinline__ LeanSrc gam_src(const RowsDev& R, const GaLeafArgs& L, int par) {
  return LeanSrc{L.ga_bpart + (int64_t)par * R.ga_nrec * PART_STRIDE, PART_STRIDE, R.ga_nrec, L.def_loc + (int64_t)par * 4 * MAX_DEFERRED};
}

// One tile into registers with ORDINARY loads (the single-chain kernel's hand-counted `global_load_dwordx4` + `vmcnt(N)` keep two
// tiles in flight across the loop, but a register with such a load pending must never be spilled -- tests/test_abi.py -- and NC
// sets of accumulators leave the allocator no such guarantee; here a spill costs time, never correctness, and a launch bound by its
// arithmetic with twelve waves per CU does not need the deeper prefetch: the other waves cover a wave's wait)
template <int DX>
__device__ __forceinline__ void gam_load(const double* base /* first element of the tile */, const int8_t* ybase, int lane,
                                         typename GaTileSel<DX>::type& t) {
  const ga_v2d* p = reinterpret_cast<const ga_v2d*>(base) + lane;
#pragma unroll
  for (int k = 0; k < DX; ++k) t.c[k] = p[k * WAVE];
  t.y = *reinterpret_cast<const uint16_t*>(ybase + 2 * lane);
}

// The seven planes of a packed tile (rows_pack.h; GA_PACKED_LOADS of rows_ga_kernel.h spells the same offsets) with ORDINARY loads,
// for the reason above: six planes of four dwords per lane, 1 KiB apart, then the plane of one dword per lane.
__device__ __forceinline__ void gam_load_packed(const uint32_t* base /* first dword of the tile */, int lane, GaTileRegsP& t) {
  const ga_v4u* p = reinterpret_cast<const ga_v4u*>(base) + lane;
#pragma unroll
  for (int k = 0; k < 6; ++k) t.p[k] = p[k * WAVE];
  t.last = base[6 * 4 * WAVE + lane];
}

// The same two requests for the paired launch's loop (SH), from a SCALAR tile address (`gam_uniform`: the compiler then adds the
// lane's byte offset where the loads are issued, instead of keeping `base + lane` of the whole array as a per-lane 64-bit address
// across the loop and multiplying the tile index into it per lane).  The global address space is spelled out: an address that
// was an integer is otherwise a flat one.
typedef const __attribute__((address_space(1))) char gam_gc;
__device__ __forceinline__ uint64_t gam_uniform(uint64_t a) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(a & 0xffffffffull));
}
template <int DX>
__device__ __forceinline__ void gam_load_s(uint64_t tile, uint64_t ytile, uint32_t lane, typename GaTileSel<DX>::type& t) {
  tile = gam_uniform(tile); ytile = gam_uniform(ytile);
  gam_gc* b = (gam_gc*)tile + lane * 16u;
#pragma unroll
  for (int k = 0; k < DX; ++k) t.c[k] = *(const __attribute__((address_space(1))) ga_v2d*)(b + k * (16 * WAVE));
  t.y = *(const __attribute__((address_space(1))) uint16_t*)((gam_gc*)ytile + lane * 2u);
}
__device__ __forceinline__ void gam_load_packed_s(uint64_t tile, uint32_t lane, GaTileRegsP& t) {
  tile = gam_uniform(tile);
  gam_gc* b = (gam_gc*)tile + lane * 16u;
#pragma unroll
  for (int k = 0; k < 6; ++k) t.p[k] = *(const __attribute__((address_space(1))) ga_v4u*)(b + k * (16 * WAVE));
  t.last = *(const __attribute__((address_space(1))) uint32_t*)((gam_gc*)tile + 6 * 16 * WAVE + lane * 4u);
}

// Row k of a lane under BOTH coefficient vectors of a paired launch (SH), the two chains side by side: a wave that evaluates one
// row under one vector has ONE dependent fp64 chain in flight (logit_row: ~40 operations, each waiting for the one before), and
// sixteen such waves per CU leave the pipe idle most of the time (tools/fp64_rate_lab.hip).  The same row under the two vectors
// is two independent chains that share their x operands -- logit_row2 issues them statement by statement next to each other --
// and needs one row's x only: the other row of the lane waits in `xx`, no second set of x registers is live.
// Per (chain, row) the operations and their order are ga_tile's (eta summed over d = 0 .. 7 from 0.0, logit_row2 bitwise
// logit_row, the mask, acc[d] = fma(r, x[d], acc[d])); neither chain reads a value of the other.
template <int K>
__device__ __forceinline__ void gam_row_pair(const double (&x)[8][2], uint32_t yb, const double (&beta)[2][8], int nvalid, int lane,
                                             double (&acc)[2][8], double (&lp)[2]) {
  double eta[2] = {0.0, 0.0}, yk[2], l[2], rr[2];
#pragma unroll
  for (int d = 0; d < 8; ++d) { eta[0] = fma(x[d][K], beta[0][d], eta[0]); eta[1] = fma(x[d][K], beta[1][d], eta[1]); }
  yk[0] = yk[1] = (double)((yb >> (8 * K)) & 0xffu);
  logit_row2(eta, yk, l, rr);
  // lane * 2 + K < nvalid (only the zero-padded last tile of a group has rows to mask), on the lane's byte offset into a 16 B-per-lane
  // plane, which the request holds in a register anyway, against a scalar
  const bool in = (uint32_t)lane * 16u < (uint32_t)((nvalid - K + 1) >> 1) * 16u;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    lp[c] += in ? l[c] : 0.0;
    rr[c] = in ? rr[c] : 0.0;
  }
#pragma unroll
  for (int d = 0; d < 8; ++d) { acc[0][d] = fma(rr[0], x[d][K], acc[0][d]); acc[1][d] = fma(rr[1], x[d][K], acc[1][d]); }
}

// D = 8 covariates, two rows per lane, two tile buffers per wave; DX stored columns (7: the intercept column is not stored).  Grid: GAM_MAXC control workgroups + G group workgroups; block: the W waves of the
// model's layout (a wave's chunk of tiles is fixed when the model is created).
// Edge pairing (SH) runs at FOUR waves per SIMD: GAM_MAXC + G workgroups of W waves are then resident at once, as the plain
// launch's are (rows_ga_kernel.h: "G workgroups of W waves must all be resident"; at three waves per SIMD 1024 of the benchmark's
// 1256 workgroups were, and the rest ran as a second round on a nearly empty chip).  128 registers hold ONE tile buffer and the
// rows of a lane one after the other, each under both coefficient vectors at once (gam_row_pair): a tile is decoded into `xx`,
// row 0 is evaluated, the wave's next tile is requested into the same registers, and row 1 is evaluated while it arrives.  PK (SH only): the tiles are the packed ones the chain's own
// launch streams (R.Xp, 6400 B per tile instead of 7296), decoded and patched exactly as k_rows_ga does.
template <int NC, int OCC, int DX, bool SH = false, int PK = 0>
__global__ __launch_bounds__(64 * GA_MAXW, OCC) void k_rows_ga_multi(ModelDev md, GaMultiArgs<NC, SH> ma) {
  constexpr int D = 8, RPL = 2, SPAN = WAVE * RPL, PIPE = 2;
  static_assert(!SH || NC == 2, "edge pairing: the chain's leaf and one shadow leaf");
  static_assert(!SH || OCC == 4, "edge pairing: four waves per SIMD, the whole grid resident");
  static_assert(!PK || (SH && DX == 7), "packed tiles: the edge-pairing launch of a model with seven stored columns");
  constexpr bool ONE = SH;   // one tile buffer, re-requested ahead of the arithmetic; rows one after the other
  typedef GaMultiArgs<NC, SH> Args;
  typedef typename GaTileSel<DX, PK>::type Tile;
  const RowsDev& R = md.lg;
  if ((int)blockIdx.x < GAM_MAXC) {   // control workgroups
    int ci = -1;
#pragma unroll
    for (int c = 0; c < NC; ++c) ci = (int)blockIdx.x == ma.c[c].slot ? c : ci;
    if (ci < 0) return;
    const GaLeafArgs& L = ma.c[ci];
    if (L.fold & GA_FOLD_CTL) control_lean(md, L.A, L.cio, L.cj, L.cd, L.Emax, L.max_depth, L.st, L.cseq, gam_src(R, L, L.par ^ 1));
    return;
  }
  const int g = (int)blockIdx.x - GAM_MAXC;
#ifdef NUTS_KTIMING
  const long long tk_top = tick_real();   // (lab build, tools/edge_pair_ticks.py: when this workgroup started)
#endif
  const int rev = ma.rev;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6), W = (int)blockDim.x >> 6;
  __shared__ double s_acc[NC][GA_MAXW][2][D + 1];   // [chain][wave][first / second half of its tiles][d/dbeta, log-lik]
  __shared__ double s_red[NC][NDOT];
  __shared__ double s_cp[GA_MAXCHUNK][PART_STRIDE];
  __shared__ int s_info[NC][4];
  __shared__ double s_keep[NC][5][WAVE];            // the tail wave's per-lane prologue values of each chain
  __shared__ double s_beta[NC][D];                  // beta_g of each chain (written by the chain's wave, read by all into scalar registers)
  __shared__ __attribute__((aligned(16))) char s_args[(sizeof(Args) + 15) / 16 * 16];

  // ---- geometry of this wave's stream (as k_rows_ga) ----
  int T; int64_t ng, cbase;
  int tg0;   // packed tiles: index of the group's first tile in the per-tile exception table
  if (R.ga_T_uni > 0) { T = R.ga_T_uni; ng = R.ga_ng_uni; cbase = (int64_t)(g * W + w) * (PK ? R.ga_pstride_uni : R.ga_cstride_uni); tg0 = g * T; }
  else {
    tg0 = __builtin_amdgcn_readfirstlane(R.ga_tile0[g]);
    T = __builtin_amdgcn_readfirstlane(R.ga_tile0[g + 1]) - tg0;
    ng = __builtin_amdgcn_readfirstlane((int)(R.gptr[g + 1] - R.gptr[g]));
    const int64_t cb = (PK ? R.ga_pcoff : R.ga_coff)[g * W + w];
    cbase = ((int64_t)__builtin_amdgcn_readfirstlane((int)(cb >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(cb & 0xffffffffll));
  }
  const int c0 = (int)((int64_t)w * T / W), c2 = (int)((int64_t)(w + 1) * T / W);
  const int n = c2 - c0;
  const int nA = (n + 1) / 2;
  const int nsw = rev ? n - nA : nA;
  constexpr int64_t TS = PK ? RP_TILE_DWORDS : (int64_t)DX * SPAN;   // doubles per tile (packed: dwords)
  auto local_at = [&](int i) { return rev ? (i < nsw ? nA + i : i - nsw) : i; };
  auto tile_at = [&](int i) { return cbase + (int64_t)local_at(i) * TS; };
  const int l_last = (c2 == T) ? n - 1 : -1;
  const int n_last = (int)(ng - (int64_t)(T - 1) * SPAN);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int dd = 0; dd <= D; ++dd) { s_acc[c][w][0][dd] = 0.0; s_acc[c][w][1][dd] = 0.0; }
  }
  {   // the chains' arguments -> LDS: the tail reads them from there (nothing of them stays in scalar registers across the stream)
    static_assert(alignof(Args) == 8 && sizeof(Args) % 8 == 0, "kernarg layout: the second argument follows the model at the next multiple of 8");
    const uint2* ka = (const uint2*)__builtin_amdgcn_kernarg_segment_ptr() + (sizeof(ModelDev) + 7) / 8;
    for (int t = tid; t < (int)(sizeof(Args) / 8); t += (int)blockDim.x) reinterpret_cast<uint2*>(s_args)[t] = ka[t];
  }

  // ---- prologue: chain c's by wave c mod W (the wave that will finish the chain): mu', sigma' of its leaf, z' of this group,
  // beta_g -> LDS.  Unlike the single-chain kernel no tile is in flight yet: NC prologues with hand-counted loads pending would
  // leave the register allocator no room (it spilled), and a launch that is bound by its arithmetic does not miss the overlap.
  int dead = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) dead |= load_aborted(ma.c[c].io, ma.c[c].A) ? (1 << c) : 0;
  if constexpr (SH) dead = (dead & 1) ? 3 : 0;   // (the shadow leaf ends with the tree: no ticket on either set of counters)
  if (dead == (1 << NC) - 1) return;   // every chain's tree has ended: the launch drains (no tickets)
  for (int c = w; c < NC; c += W) {
    const GaLeafArgs& L = ma.c[c];
    Leaf lf; QView qv;
    double hval0, hph0;
    if (SH && c == 1 && (L.pad & GAM_SH_FIRST)) {   // the shadow sequence's first leaf: from the chain's arena (and block partials)
      resolve_leaf(L.io, ma.c[0].A, L.j, lf, qv);
      ga_hyper<D>(R, qv, L.fold, gam_src(R, ma.c[0], ma.c[0].par ^ 1), lane, hval0, hph0);
    } else {
      resolve_leaf(L.io, L.A, L.j, lf, qv);
      ga_hyper<D>(R, qv, L.fold, gam_src(R, L, L.par ^ 1), lane, hval0, hph0);
    }
    const int dl = lane % D;
    const int iz = R.off_z + g * D + dl;
    double zq, zph, m_lane, s_lane;
    ga_z_state(qv, iz, zq, zph);
    ga_hyper_lanes<D>(R, hval0, dl, m_lane, s_lane);
    const double bl = fma(s_lane, zq, m_lane);
    if (lane < D) s_beta[c][lane] = bl;
    s_keep[c][0][lane] = hval0; s_keep[c][1][lane] = hph0; s_keep[c][2][lane] = zq; s_keep[c][3][lane] = zph; s_keep[c][4][lane] = s_lane;
  }
  __syncthreads();
  // Two tile buffers per wave (one being evaluated, one requested) up to three chains; with FOUR sets of accumulators the second
  // buffer is what pushed the allocator into spilling inside the loop (107 us per launch against 80 for three chains, rocprofv3
  // r05c): one buffer then, the wave's next tile is requested when the current one has been evaluated -- at ~1.3 us of arithmetic
  // per tile and twelve waves per CU the other waves cover the wait.
  constexpr bool TWO = NC <= 3 && !ONE;
  Tile ta, tb;
  uint64_t ea = 0;   // packed tiles: the exception range of the tile in flight (a scalar load issued with the tile)
  const int te0 = tg0 + c0;
  // (a wave without tiles requests the chunk's first tile slot anyway: the layout keeps one tile of slack behind every chunk)
  if constexpr (PK) {
    gam_load_packed(R.Xp + tile_at(0), lane, ta);
    ea = ga_exc_range(R.ga_pexc_idx, te0 + local_at(0));
  } else {
    const int64_t o0 = tile_at(0), o1 = tile_at(min(1, max(n - 1, 0)));
    gam_load<DX>(R.Xt + o0, R.y + o0 / DX, lane, ta);
    if constexpr (TWO) gam_load<DX>(R.Xt + o1, R.y + o1 / DX, lane, tb);
  }
  double beta[NC][D];   // wave-uniform: scalar registers
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int dd = 0; dd < D; ++dd) beta[c][dd] = readlane_d(s_beta[c][dd], 0);

  // ---- the stream: every tile once, every row under NC coefficient vectors ----
  {
    double acc[NC][D], lp[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      lp[c] = 0.0;
#pragma unroll
      for (int dd = 0; dd < D; ++dd) acc[c][dd] = 0.0;
    }
    int half = rev ? 1 : 0;
    auto flush = [&]() {
      // NC (D + 1) wave sums at once, each in wave_sum's association order (mvn_multi_kernel.h, wave_sum_many)
      double flat[NC * D];
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int dd = 0; dd < D; ++dd) flat[c * D + dd] = acc[c][dd];
      int idx;
      const double t = wave_sum_many<NC * D>(flat, lane, idx);
      constexpr int NVP = NC * D <= 8 ? 8 : NC * D <= 16 ? 16 : 32;
      if (lane < NVP && idx < NC * D) s_acc[idx / D][w][half][idx % D] = t;
      int idx2;
      const double t2 = wave_sum_many<NC>(lp, lane, idx2);
      constexpr int NVP2 = NC <= 1 ? 1 : NC <= 2 ? 2 : 4;
      if (lane < NVP2 && idx2 < NC) s_acc[idx2][w][half][D] = t2;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        lp[c] = 0.0;
#pragma unroll
        for (int dd = 0; dd < D; ++dd) acc[c][dd] = 0.0;
      }
      half ^= 1;
    };
    const int nm1 = n - 1;
    auto issue = [&](int i, Tile& t) {   // (unconditional: past the end it re-reads the wave's last tile)
      const int ii = min(i, nm1);
      if constexpr (PK) {
        gam_load_packed(R.Xp + tile_at(ii), lane, t);
        ea = ga_exc_range(R.ga_pexc_idx, te0 + local_at(ii));
      } else {
        const int64_t off = tile_at(ii);
        gam_load<DX>(R.Xt + off, R.y + off / DX, lane, t);
      }
    };
#define GAM_STAGE(TT, I)                                                                     \
    {                                                                                        \
      if ((I) == nsw) flush();                                                               \
      double xx[8][2];                                                                       \
      ga_unpack(TT, xx);                                                                     \
      const uint32_t yy = TT.y;                                                              \
      const int nv = local_at(I) == l_last ? n_last : SPAN;                                  \
      /* (two chains and more: the rows of a lane side by side, logit_row2 -- the launch is bound by dependent fp64 issue, not HBM) */ \
      _Pragma("unroll") for (int c = 0; c < NC; ++c) ga_tile<8, 2, (NC == 2)>(xx, yy, beta[c], nv, lane, acc[c], lp[c]); \
    }
    if constexpr (ONE) {
      // one buffer, four waves per SIMD: decode (packed: and patch) the tile into `xx`; row 0, re-request the buffer, row 1
      uint32_t ebase20 = 0;
      if constexpr (PK) ebase20 = R.ga_pack_ebase20;
      // `local_at` as one scalar select (a branch here splits the arithmetic into blocks the request cannot be pinned between)
      const int radd = rev ? nA : 0, rsub = rev ? nsw : 0;
      // (the stream's pointers as scalars of their own: read out of the model's kernel argument inside the loop, each drags the
      // sixteen-register block it was loaded with back from its spill slot, once per tile)
      uint64_t xbase = (uint64_t)(PK ? (const void*)R.Xp : (const void*)R.Xt), ybase = (uint64_t)R.y;
      const uint64_t* pexc_idx = R.ga_pexc_idx;
      const RpExc* pexc = R.ga_pexc;
      asm("" : "+s"(xbase), "+s"(ybase), "+s"(pexc_idx), "+s"(pexc));
      auto local1 = [&](int i) { return i + (i < nsw ? radd : -rsub); };
      auto issue1 = [&](int i) {   // (unconditional: past the end it re-reads the wave's last tile)
        const int loc = local1(min(i, nm1));
        const int64_t off = cbase + (int64_t)loc * TS;
        if constexpr (PK) {
          gam_load_packed_s(xbase + (uint64_t)off * 4, (uint32_t)lane, ta);
          ea = ga_exc_range(pexc_idx, te0 + loc);
        } else {
          gam_load_s<DX>(xbase + (uint64_t)off * 8, ybase + (uint64_t)(off / DX), (uint32_t)lane, ta);
        }
      };
      auto stage = [&](int i) {
        double xx[8][2];
        if constexpr (PK) {
          ga_unpack(ta, ebase20, xx);
          if ((uint32_t)(ea >> 32) != 0) ga_patch(pexc, ea, lane, xx);
        } else {
          ga_unpack(ta, xx);
        }
        const uint32_t yy = ga_ybits(ta);
        const int nv = local1(i) == l_last ? n_last : SPAN;
        // row 0 under both vectors, then the request (row 0's x registers are dead: they make room for the tile), then row 1 while
        // it arrives.  The barriers keep the request where it is written: above row 0 it would not fit 128 registers.  With eight
        // stored columns it does not fit between the rows either (33 tile registers + 16 of row 1: one reload per tile): that
        // instantiation requests behind row 1, the other waves of the SIMD cover its wait.
        constexpr bool MID = DX == 7;
        gam_row_pair<0>(xx, yy, beta, nv, lane, acc, lp);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MID) { issue1(i + 1); __builtin_amdgcn_sched_barrier(0); }
        gam_row_pair<1>(xx, yy, beta, nv, lane, acc, lp);
        if constexpr (!MID) { __builtin_amdgcn_sched_barrier(0); issue1(i + 1); }
      };
      if constexpr (PK) {
        // the wave's two halves as two loops, the mid-stream flush between them: as `if (i == nsw) flush()` inside ONE loop its
        // masks and addresses stay live across the arithmetic of every tile, and most of `beta` is then reloaded from its spill
        // lanes once per tile (61 `v_readlane` per tile against 14).  The raw kernels keep one loop: split, the seven-column one
        // reloads four values from scratch per tile of its second half.
        const int n0 = min(nsw, n);
        for (int i = 0; i < n0; ++i) stage(i);
        if (nsw < n) {
          flush();
          for (int i = nsw; i < n; ++i) stage(i);
        }
      } else {
        for (int i = 0; i < n; ++i) {
          if (i == nsw) flush();
          stage(i);
        }
      }
    } else if constexpr (TWO) {
      for (int i = 0; i < n; i += 2) {
        GAM_STAGE(ta, i)
        if (i + 1 >= n) break;
        issue(i + 2, ta);
        GAM_STAGE(tb, i + 1)
        issue(i + 3, tb);
      }
    } else {
      for (int i = 0; i < n; ++i) {
        GAM_STAGE(ta, i)
        issue(i + 1, ta);
      }
    }
#undef GAM_STAGE
    if (n > 0) flush();
  }

  // ---- tails: chain c is finished by wave c mod W; then the block partials of the chains this workgroup arrived last for ----
  const Args& Tm = *reinterpret_cast<const Args*>(s_args);
  MergePrefetch mpf;
  // (the operands of the first merge levels belong to earlier leaves: requested -- for the first chain a wave finishes -- before the
  // wave waits for the others)
  if (w < NC && !((dead >> w) & 1) && !(SH && w == 1)) {
    const GaLeafArgs& L = Tm.c[w];
    Leaf lf; QView qv;
    resolve_leaf(L.io, L.A, L.j, lf, qv);
    merge_prefetch(L.A, lf, L.j, R.off_z + g * D + lane % D, mpf);
  }
  __syncthreads();
  if constexpr (SH) {   // the shadow leaf's wave sums -> its ring entry (plain stores: the kernel boundary publishes them)
    constexpr int NR = GA_RING_DOUBLES(D);
    for (int t = tid; t < NR; t += (int)blockDim.x) Tm.ring[(int64_t)g * NR + t] = (&s_acc[1][0][0][0])[t];
  }
  for (int c = w; c < NC; c += W) {
    if ((dead >> c) & 1) { if (lane == 0) s_info[c][0] = 0; continue; }
    const GaLeafArgs& L = Tm.c[c];
    Leaf lf; QView qv;
    resolve_leaf(L.io, L.A, L.j, lf, qv);
    if (SH && c == 1) {   // (MODE_SIMPLE: the kick, q', the record, the ticket -- no leaf_post merges)
      ga_tail_wave<D, false>(R, L.A, L.io, L.ga_part, L.ga_ticket, L.def_loc, lf, g, W, L.j, L.par, L.d, s_acc[c], s_red[c], s_info[c],
                             s_keep[c][0][lane], s_keep[c][1][lane], s_keep[c][2][lane], s_keep[c][3][lane], s_keep[c][4][lane], nullptr);
      continue;
    }
    auto tail = [&](const MergePrefetch* pf) {   // (a compile-time pointer in either call: `mpf` stays in registers)
      ga_tail_wave<D, true>(R, L.A, L.io, L.ga_part, L.ga_ticket, L.def_loc, lf, g, W, L.j, L.par, L.d, s_acc[c], s_red[c], s_info[c],
                            s_keep[c][0][lane], s_keep[c][1][lane], s_keep[c][2][lane], s_keep[c][3][lane], s_keep[c][4][lane], pf);
    };
    if (c == w) tail(&mpf);
    else tail(nullptr);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (!s_info[c][0]) continue;            // (workgroup-uniform)
    ga_block_partial<D>(R, Tm.c[c].ga_part, Tm.c[c].ga_bpart, Tm.c[c].par, g, true, s_info[c], s_cp);
    __syncthreads();
  }
#ifdef NUTS_KTIMING
  if constexpr (SH) {   // start and retirement of every group workgroup of the last paired launch (nuts_model_debug_ticks sums them up)
    __syncthreads();
    if (tid == 0 && g < EP_TICK_WG) { md.ticks[64 + 2 * g] = tk_top; md.ticks[64 + 2 * g + 1] = tick_real(); }
  }
#endif
}
