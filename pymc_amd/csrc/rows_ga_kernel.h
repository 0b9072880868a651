// Group-aligned row pass for the hierarchical Bernoulli-logit node: ONE launch per leapfrog step.
//
// The span-partitioned pass (rows_kernel.h) balances rows over waves regardless of the group structure, which leaves
// the gradient of a group's z elements scattered over several workgroups; an O(n) kernel (kernel B, kernels.h) has to
// run between two row passes to combine them, kick the momenta and form the tree's dot products -- 10 us of pure
// latency per leapfrog on the benchmark shape (20 % of the step).  When the groups are large and balanced (C2-L: 1248
// groups x 4000 rows) the pass is partitioned BY GROUP instead:
//
//   * workgroup g (W waves) streams exactly the rows of group g.  X is tiled per group ([tiles][D][SPAN], last tile of a
//     group zero-padded and masked), so no tile is shared between workgroups and there are no "mixed" spans; all G
//     workgroups are resident at once (W is chosen so that G W waves fit the chip).
//   * after its last tile the workgroup holds the complete d logp / d beta_g (W wave partials combined through LDS in
//     wave order) and finishes the group's D z elements itself: gradient, second half kick p' = p_half + eps/2 g',
//     v' = M^-1 p', q' store, and the tree-merge dot products of `leaf_post` (kernels.h) restricted to its D elements.
//   * what must cross workgroups is small: per group one record {logp, d/dmu[D], d/dsigma[D], dots}.  Records are
//     written write-through (agent-scope stores), the workgroup takes a ticket on its block's arrival counter (blocks of
//     ga_bsz consecutive groups), and the block's last arriver sums the block's records in group order into a block
//     partial.  No floating-point atomics, no dependence on arrival order: the sums are in fixed order, the ticket only
//     decides WHO does them.  (Hand-off form: MI355X guide, "sc1 payload -> s_waitcnt vmcnt(0) -> ticket; consumer reads
//     with agent-scope loads".)
//   * the next leaf's launch starts from the ga_nblk block partials exactly as it used to start from kernel B's
//     per-workgroup partials: every wave finishes mu' / sigma' in its prologue (rows_hyper_fold_elem), workgroup 0
//     runs the control work of the previous leaf (control_lean) -- both read the block partials of the PREVIOUS launch's
//     parity, this launch writes the other one.
//
// Arena writes of a speculative leaf (one that starts while its predecessor's control work decides to stop the tree) go
// to the slot of a state nobody will read; arrival counters reset themselves (last arriver) and, because the `aborted`
// flag can flip while a launch is in flight, once more at the end of every draw (k_draw_finish).
#pragma once
#include "rows_kernel.h"
#include "rows_pack.h"

// the local part of a hyper-parameter element: what kernel B evaluates through the interpreter on the lean path
// (transform_full + its own prior), here in closed form (the spec compiler only selects this path for mu ~ Normal,
// sigma ~ HalfNormal with constant parameters)
__device__ __forceinline__ void ga_def_local(const RowsDev& R, bool is_mu, double qn, double& gx, double& dxdq, double& dj, double& lp) {
  if (is_mu) {
    const double r = qn - R.mu_c[0];
    const double z = r * R.mu_c[1];
    lp = -0.5 * z * z - R.mu_c[2] + (-0.91893853320467274178);
    gx = -z * R.mu_c[1]; dxdq = 1.0; dj = 0.0;
  } else {
    double x, lj;
    if (R.sigma_tr == NUTS_TR_LOG) { x = exp(qn); dxdq = x; lj = qn; dj = 1.0; }   // transforms.py:880-891
    else { x = qn; dxdq = 1.0; lj = 0.0; dj = 0.0; }
    const double z = x * R.sg_c[0];
    double lpf = -0.5 * z * z - R.sg_c[1] + (-0.22579135264472743236);
    double g = -z * R.sg_c[0];
    if (!(x >= 0)) { lpf = -INFINITY; g = 0.0; }                                   // continuous.py:909-916 support check
    gx = g; lp = lj + lpf;
  }
}

// X tile at element offset `xoff` of Xt ([D][SPAN] doubles; its y bytes at xoff / D): lane l holds rows RPL*l .. RPL*l+RPL-1
template <int D, int RPL>
__device__ __forceinline__ void ga_load(const RowsDev& R, int64_t xoff, int lane, double (&x)[D][RPL], uint32_t& ybits) {
  constexpr int SPAN = WAVE * RPL;
  const double* tile = R.Xt + xoff + lane * RPL;
  const int8_t* yp = R.y + xoff / D + lane * RPL;
  if (RPL == 2) ybits = *reinterpret_cast<const uint16_t*>(yp);
  else ybits = *reinterpret_cast<const uint32_t*>(yp);
#pragma unroll
  for (int d = 0; d < D; ++d) {
#pragma unroll
    for (int k = 0; k < RPL; k += 2) {
      const double2 a = *reinterpret_cast<const double2*>(tile + d * SPAN + k);
      x[d][k] = a.x; x[d][k + 1] = a.y;
    }
  }
}

// ---- hand-counted tile loads (D = 8, two rows per lane) ----------------------------------------------------------------------
// hipcc cannot keep a tile in flight across the loop: it drains every outstanding load (`s_waitcnt vmcnt(0)`) at the loop header
// before it lets the next request go (the destination registers of the buffers double as its address temporaries), so the
// stream ran with ONE tile per wave in flight however deep the source-level pipeline was.  The nine loads of a tile are
// therefore issued from one asm statement (scalar base + per-lane offset, no vector address arithmetic) and waited for with a
// counted `vmcnt(N)`, N = 9 x (tiles requested after the one needed).  Form (ii) of the guide's inline-asm rules: "=&v" loads,
// and a wait statement that names every destination "+v" ahead of the first consumer.
typedef double ga_v2d __attribute__((ext_vector_type(2)));
struct GaTileRegs { ga_v2d c[8]; uint32_t y; };

__device__ __forceinline__ void ga_issue8(const double* base /* wave-uniform: first element of the tile */, const int8_t* ybase,
                                          uint32_t voff16, uint32_t voff2, GaTileRegs& t) {
  const double* base2 = base + 512;   // columns 4 .. 7 (the immediate offset field is 13 bits)
  asm volatile(
      "s_nop 4\n\t"
      "global_load_dwordx4 %0, %9, %10\n\t"
      "global_load_dwordx4 %1, %9, %10 offset:1024\n\t"
      "global_load_dwordx4 %2, %9, %10 offset:2048\n\t"
      "global_load_dwordx4 %3, %9, %10 offset:3072\n\t"
      "global_load_dwordx4 %4, %9, %11\n\t"
      "global_load_dwordx4 %5, %9, %11 offset:1024\n\t"
      "global_load_dwordx4 %6, %9, %11 offset:2048\n\t"
      "global_load_dwordx4 %7, %9, %11 offset:3072\n\t"
      "global_load_ushort %8, %12, %13"
      : "=&v"(t.c[0]), "=&v"(t.c[1]), "=&v"(t.c[2]), "=&v"(t.c[3]), "=&v"(t.c[4]), "=&v"(t.c[5]), "=&v"(t.c[6]), "=&v"(t.c[7]), "=&v"(t.y)
      : "v"(voff16), "s"(base), "s"(base2), "v"(voff2), "s"(ybase)
      : "memory");
}

template <int N>
__device__ __forceinline__ void ga_wait8(GaTileRegs& t) {   // at most N loads may still be outstanding; `t` is complete afterwards
  asm volatile("s_waitcnt vmcnt(%9)"
               : "+v"(t.c[0]), "+v"(t.c[1]), "+v"(t.c[2]), "+v"(t.c[3]), "+v"(t.c[4]), "+v"(t.c[5]), "+v"(t.c[6]), "+v"(t.c[7]), "+v"(t.y)
               : "i"(N));
}

// ---- the same with SEVEN stored columns: column 0 of X is identically 1 (the intercept) and is not stored ----
// Detected when the model is built (engine.hip): the tiles are [7][SPAN], 7 KiB instead of 8, and the kernel multiplies by the
// literal 1.0 -- fma(1, beta_0, 0) and fma(r, 1, acc) are what the stored column would have produced, bit for bit.  The row
// pass moves 57 B per row instead of 65 (the ALGORITHMIC figure of SURVEY 8d stays 69: bench.py prices both).
struct GaTileRegs7 { ga_v2d c[7]; uint32_t y; };

__device__ __forceinline__ void ga_issue8(const double* base, const int8_t* ybase, uint32_t voff16, uint32_t voff2, GaTileRegs7& t) {
  const double* base2 = base + 512;   // stored columns 4 .. 6
  asm volatile(
      "s_nop 4\n\t"
      "global_load_dwordx4 %0, %8, %9\n\t"
      "global_load_dwordx4 %1, %8, %9 offset:1024\n\t"
      "global_load_dwordx4 %2, %8, %9 offset:2048\n\t"
      "global_load_dwordx4 %3, %8, %9 offset:3072\n\t"
      "global_load_dwordx4 %4, %8, %10\n\t"
      "global_load_dwordx4 %5, %8, %10 offset:1024\n\t"
      "global_load_dwordx4 %6, %8, %10 offset:2048\n\t"
      "global_load_ushort %7, %11, %12"
      : "=&v"(t.c[0]), "=&v"(t.c[1]), "=&v"(t.c[2]), "=&v"(t.c[3]), "=&v"(t.c[4]), "=&v"(t.c[5]), "=&v"(t.c[6]), "=&v"(t.y)
      : "v"(voff16), "s"(base), "s"(base2), "v"(voff2), "s"(ybase)
      : "memory");
}

template <int N>
__device__ __forceinline__ void ga_wait8(GaTileRegs7& t) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(t.c[0]), "+v"(t.c[1]), "+v"(t.c[2]), "+v"(t.c[3]), "+v"(t.c[4]), "+v"(t.c[5]), "+v"(t.c[6]), "+v"(t.y)
               : "i"(N));
}

// tile registers -> the [8][2] operand of ga_tile
__device__ __forceinline__ void ga_unpack(const GaTileRegs& t, double (&xx)[8][2]) {
#pragma unroll
  for (int dd = 0; dd < 8; ++dd) { xx[dd][0] = t.c[dd].x; xx[dd][1] = t.c[dd].y; }
}
__device__ __forceinline__ void ga_unpack(const GaTileRegs7& t, double (&xx)[8][2]) {
  xx[0][0] = 1.0; xx[0][1] = 1.0;
#pragma unroll
  for (int dd = 1; dd < 8; ++dd) { xx[dd][0] = t.c[dd - 1].x; xx[dd][1] = t.c[dd - 1].y; }
}
__device__ __forceinline__ uint32_t ga_ybits(const GaTileRegs& t) { return t.y; }
__device__ __forceinline__ uint32_t ga_ybits(const GaTileRegs7& t) { return t.y; }

// ---- the seven stored columns as lossless 57-bit values (rows_pack.h): 6400 B per tile instead of 7296, 7 loads, 25 registers ----
// Every load reads one contiguous block: six 1 KiB planes of four dwords per lane and one 256 B plane of one (a lane's 25 dwords:
// the low dwords of its 14 slots, then its 352-bit string of high fields + y bits).  Chosen when the model is built (engine.hip,
// build_rows_group); the decode rebuilds the stored fp64 bit for bit, so ga_tile sees the operands the raw tile would have given it.
typedef uint32_t ga_v4u __attribute__((ext_vector_type(4)));
struct GaTileRegsP { ga_v4u p[6]; uint32_t last; };

struct GaPackOff { uint32_t v16, v4; };   // per-lane byte offsets into the 16 / 4 B-per-lane planes

// the seven loads of a packed tile: %0 .. %6 the destinations, %7 / %8 the lane's offsets into the 16 / 4 B-per-lane planes,
// %9 / %10 the tile's first dword and dword 1024 (ONE text for both requests below: they differ in their ordering operands only)
#define GA_PACKED_LOADS                                   \
  "s_nop 4\n\t"                                           \
  "global_load_dwordx4 %0, %7, %9\n\t"                    \
  "global_load_dwordx4 %1, %7, %9 offset:1024\n\t"        \
  "global_load_dwordx4 %2, %7, %9 offset:2048\n\t"        \
  "global_load_dwordx4 %3, %7, %9 offset:3072\n\t"        \
  "global_load_dwordx4 %4, %7, %10\n\t"                   \
  "global_load_dwordx4 %5, %7, %10 offset:1024\n\t"       \
  "global_load_dword %6, %8, %10 offset:2048"

__device__ __forceinline__ void ga_issue8(const uint32_t* base /* wave-uniform: first dword of the tile */, const GaPackOff& vo, GaTileRegsP& t) {
  const uint32_t* base2 = base + 1024;   // planes 4 .. 6 (the immediate offset field is 13 bits, signed)
  asm volatile(
      GA_PACKED_LOADS
      : "=&v"(t.p[0]), "=&v"(t.p[1]), "=&v"(t.p[2]), "=&v"(t.p[3]), "=&v"(t.p[4]), "=&v"(t.p[5]), "=&v"(t.last)
      : "v"(vo.v16), "v"(vo.v4), "s"(base), "s"(base2)
      : "memory");
}

// The same request inside the streaming loop, where `t` is being REPLACED.  An asm statement orders memory operations only, so
// nothing in the language keeps a register-only consumer of the OLD tile above it; were one scheduled below, the old tile would
// still be live at the request, the new one would get other registers and be copied into the loop-carried ones at the back-edge,
// while its loads are in flight.  The sums the stage on the old tile produced are therefore named as inputs: every instruction
// that reads the old tile comes before the request.  The raw requests above carry no such operands and rely on the scheduler
// alone; tests/test_rows_ga_tile_registers.py holds all of them to it on the built code object (each tile in flight keeps ONE
// set of destination registers).
__device__ __forceinline__ void ga_issue8(const uint32_t* base, const GaPackOff& vo, GaTileRegsP& t, const double (&acc)[8], double lp) {
  const uint32_t* base2 = base + 1024;
  asm volatile(
      GA_PACKED_LOADS
      : "=&v"(t.p[0]), "=&v"(t.p[1]), "=&v"(t.p[2]), "=&v"(t.p[3]), "=&v"(t.p[4]), "=&v"(t.p[5]), "=&v"(t.last)
      : "v"(vo.v16), "v"(vo.v4), "s"(base), "s"(base2),
        "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]), "v"(acc[4]), "v"(acc[5]), "v"(acc[6]), "v"(acc[7]), "v"(lp)
      : "memory");
}

template <int N>
__device__ __forceinline__ void ga_wait8(GaTileRegsP& t) {
  asm volatile("s_waitcnt vmcnt(%7)"
               : "+v"(t.p[0]), "+v"(t.p[1]), "+v"(t.p[2]), "+v"(t.p[3]), "+v"(t.p[4]), "+v"(t.p[5]), "+v"(t.last)
               : "i"(N));
}

// decode: low dword as stored, high dword from the slot's 25-bit field (at bit 25 slot of the lane's string: one funnel shift with
// a compile-time amount) and the window's base exponent
// (every element is named with compile-time indices: an array built from the members would be read back from the tile as
// ONE wide load, and the tile would then live in scratch)
template <int DW> __device__ __forceinline__ uint32_t ga_pdw(const GaTileRegsP& t) {   // dword DW of the lane's 25
  if constexpr (DW < 24) return t.p[DW >> 2][DW & 3]; else return t.last;
}
template <int S> __device__ __forceinline__ uint32_t ga_plo(const GaTileRegsP& t) { return ga_pdw<S>(t); }
template <int Q> __device__ __forceinline__ uint32_t ga_phi(const GaTileRegsP& t) { return ga_pdw<RP_SLOTS + Q>(t); }
template <int S> __device__ __forceinline__ double ga_pslot(const GaTileRegsP& t, uint32_t ebase20) {
  constexpr int q = (RP_FIELD_BITS * S) >> 5, r = (RP_FIELD_BITS * S) & 31;
  uint32_t f;
  if constexpr (r + RP_FIELD_BITS <= 32) f = ga_phi<q>(t) >> r;
  else f = __builtin_amdgcn_alignbit(ga_phi<q + 1>(t), ga_phi<q>(t), r);
  return __hiloint2double((int)rp_decode_hi(f, ebase20), (int)ga_plo<S>(t));
}
__device__ __forceinline__ void ga_unpack(const GaTileRegsP& t, uint32_t ebase20, double (&xx)[8][2]) {
  xx[0][0] = 1.0; xx[0][1] = 1.0;
#define GA_PCOL(C) xx[1 + C][0] = ga_pslot<2 * C>(t, ebase20); xx[1 + C][1] = ga_pslot<2 * C + 1>(t, ebase20);
  GA_PCOL(0) GA_PCOL(1) GA_PCOL(2) GA_PCOL(3) GA_PCOL(4) GA_PCOL(5) GA_PCOL(6)
#undef GA_PCOL
}
__device__ __forceinline__ uint32_t ga_ybits(const GaTileRegsP& t) { return ((t.last >> 30) & 1u) | ((t.last >> 31) << 8); }

// Exceptions (values outside the window): the raw bits of (lane, slot) replace the decoded placeholder.  Everything here is
// wave-uniform control and scalar loads (constant address space: lgkmcnt-counted, the vector-load count is not disturbed).
typedef const __attribute__((address_space(4))) uint64_t ga_k64;
typedef const __attribute__((address_space(4))) ga_v4u ga_k128;   // one RpExc: {tile, lane | slot << 8, low dword, high dword}
__device__ __forceinline__ uint64_t ga_exc_range(const uint64_t* idx, int tile) { return ((ga_k64*)idx)[tile]; }   // start | count << 32
__device__ __forceinline__ void ga_patch(const RpExc* list, uint64_t range, int lane, double (&xx)[8][2]) {
  const uint32_t e0 = (uint32_t)range, e1 = e0 + (uint32_t)(range >> 32);
  for (uint32_t e = e0; e < e1; ++e) {
    const ga_v4u x = ((ga_k128*)list)[e];
    const int L = (int)(x.y & 0xffu), sl = (int)(x.y >> 8);
    const double v = __hiloint2double((int)x.w, (int)x.z);
#pragma unroll
    for (int s = 0; s < RP_SLOTS; ++s) {
      const bool hit = lane == L && sl == s;
      xx[1 + (s >> 1)][s & 1] = hit ? v : xx[1 + (s >> 1)][s & 1];
    }
  }
}

template <int DX, int PK = 0> struct GaTileSel { typedef GaTileRegs type; };
template <> struct GaTileSel<7, 0> { typedef GaTileRegs7 type; };
template <> struct GaTileSel<7, 1> { typedef GaTileRegsP type; };

// one tile of SPAN = 64 RPL rows: forward (eta, log-lik) + backward (d/dbeta) in registers
// ILV: the rows of a lane may be interleaved by the scheduler (rows_gal_kernel.h: a dependent fp64 fma issues every ~24 cycles, and
// a wave that holds ONE tile has the registers for two rows' temporaries; per row the operations and their order are the same)
template <int D, int RPL, bool ILV = false>
__device__ __forceinline__ void ga_tile(const double (&x)[D][RPL], uint32_t yb, const double (&beta)[D], int nvalid, int lane,
                                        double (&acc)[D], double& lp) {
  if constexpr (ILV && RPL == 2) {
    double eta[2] = {0.0, 0.0}, yk[2], l[2], rr[2];
#pragma unroll
    for (int d = 0; d < D; ++d) { eta[0] = fma(x[d][0], beta[d], eta[0]); eta[1] = fma(x[d][1], beta[d], eta[1]); }
    yk[0] = (double)(yb & 0xffu); yk[1] = (double)((yb >> 8) & 0xffu);
    logit_row2(eta, yk, l, rr);
    // (row 0's contributions enter the lane's sums before row 1's, as in the loop below)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bool in = lane * 2 + k < nvalid;
      lp += in ? l[k] : 0.0;
      rr[k] = in ? rr[k] : 0.0;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) { acc[d] = fma(rr[0], x[d][0], acc[d]); acc[d] = fma(rr[1], x[d][1], acc[d]); }
    return;
  }
#pragma unroll
  for (int k = 0; k < RPL; ++k) {
    double eta = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) eta = fma(x[d][k], beta[d], eta);
    double l, rr;
    logit_row(eta, (double)((yb >> (8 * k)) & 0xffu), l, rr);
    const bool in = lane * RPL + k < nvalid;   // (only the zero-padded last tile of a group has rows to mask)
    lp += in ? l : 0.0;
    rr = in ? rr : 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = fma(rr, x[d][k], acc[d]);
    // rows are finished one after the other: interleaving the two rows of a lane would double the live temporaries of the
    // exp / log1p / reciprocal sequences, and the registers are better spent on tiles in flight
    if constexpr (!ILV) __builtin_amdgcn_sched_barrier(0);
  }
}

#define GA_MAXW 4
#define GA_MAXCHUNK 8      // the block reduce sums chunks of 8 consecutive groups (ga_bsz <= 64)
#define GA_F_NOTAIL 1      // ga_flags, TIMING EXPERIMENTS ONLY: stop after the stream (results are wrong)
// Edge pairing: a launch may evaluate, next to its own leaf, the next leapfrog of the trajectory's OTHER end on the
// same tiles (rows_ga_multi_kernel.h, SH) and park that leaf's finished wave sums -- `s_acc`, all a tail needs from the stream --
// in a ring entry of GA_RING_DOUBLES(D) doubles per group; when the tree reaches that leaf, `k_rows_ga_replay` below starts from
// the entry instead of streaming X.
#define GA_RING_LEAVES 64
#define GA_RING_DOUBLES(D) (GA_MAXW * 2 * ((D) + 1))

// Register budget: four waves per SIMD (128 VGPRs), two tiles in flight per wave.
// G workgroups of W waves must all be resident: 16 waves per CU >= W (G / CUs).
struct GaArgs;
template <int D>
__device__ __forceinline__ void ga_tail(const GaArgs& T, int g, double (&s_acc)[4][2][D + 1], double (&s_red)[NDOT],
                                        double (&s_cp)[8][PART_STRIDE], int (&s_info)[4], double (&s_keep)[5][WAVE]);

// The arguments travel as ONE struct: the tail of the kernel reads them from an LDS copy of the kernarg segment (made while the
// first tile is in flight), so that nothing the tail needs -- a few dozen pointers and scalars -- has to stay in scalar
// registers across the streaming loop.  (They did: 100+ SGPRs, spilled into VGPR lanes, spilled on into scratch; and a scratch
// reload inside the loop waits, in order, for every tile load issued before it -- the prefetch was gone.)
struct GaArgs {
  ModelDev md; ArenaDev A; EvalIO io;
  int j, rev, fold, par, d, max_depth;
  double Emax;
  HostStatus* st;
  // `fold` bit 0: workgroup 0 does control work -- of leaf (cio, cj, cd), publishing sequence number cseq when it is the last
  // leaf of a doubling.  Inside a doubling that is leaf j - 1 of the same doubling; the FIRST leaf of a doubling queued by the
  // host's look-ahead carries the control work of the previous doubling's last leaf (which would otherwise be a launch of its
  // own, 10-35 us between two row passes).  `fold` bit 1: the source state of this leaf is the leaf of the previous launch, so
  // mu' / sigma' come from that launch's block partials (always so inside a doubling; across doublings only when the tree keeps
  // growing on the same side -- otherwise the source is an older edge state whose entries are complete in the arena).
  EvalIO cio;
  int cj, cd, cseq, cpad;
};
#define GA_FOLD_CTL 1
#define GA_FOLD_SRC 2
#include "rows_aux.h"

// mu', sigma' of this leaf: lane l gets q' (`hval0`) and p_half (`hph0`) of hyper-parameter element l mod 2D.  GA_FOLD_SRC: the source
// state is the leaf of the previous launch, whose mu / sigma gradient is finished here from that launch's records (`prev`: the
// model's, lean_src, or a group member's own, gam_src).
template <int D>
__device__ __forceinline__ void ga_hyper(const RowsDev& R, const QView& qv, int fold, const LeanSrc prev, int lane, double& hval0, double& hph0) {
  if (fold & GA_FOLD_SRC) {
    rows_hyper_fold_elem<D>(R, prev.part, prev.stride, prev.nblk, prev.def_loc, qv, lane, hval0, hph0);
  } else {
    const int e = lane % (2 * D);
    const int i = e < D ? R.off_mu + e : R.off_sigma + (e - D);
    if (qv.composed) { hph0 = qv.p_half(i); hval0 = fma(qv.eps, qv.var[i] * hph0, qv.q[i]); }
    else { hph0 = 0.0; hval0 = qv.q[i]; }
  }
}

// ---- a group's prologue and everything after its stream: ONE copy for k_rows_ga, k_rows_ga_multi (rows_ga_multi_kernel.h) and
// k_rows_gal (rows_gal_kernel.h) -- a chain in a group runs the code below on its own buffers, so it is bitwise the chain alone by
// construction; the group-block pass (rows_gb_kernel.h) shares the pieces that are not about records crossing workgroups ----

// z' and p_half of element `iz` of this leaf
__device__ __forceinline__ void ga_z_state(const QView& qv, int iz, double& zq, double& zph) {
  if (qv.composed) { zph = fma(qv.half, qv.g[iz], qv.p[iz]); zq = fma(qv.eps, qv.var[iz] * zph, qv.q[iz]); }
  else { zph = 0.0; zq = qv.q[iz]; }
}

// mu_d', sigma_d' (constrained) of coordinate d = `dl` from the lanes of ga_hyper; beta_g,d = fma(s_lane, z', m_lane)
template <int D>
__device__ __forceinline__ void ga_hyper_lanes(const RowsDev& R, double hval0, int dl, double& m_lane, double& s_lane) {
  m_lane = __shfl(hval0, dl);
  const double sraw = __shfl(hval0, D + dl);
  s_lane = R.sigma_tr == NUTS_TR_LOG ? exp(sraw) : sraw;
}

// z ~ Normal(mu0, s0) in closed form (continuous.py:526-532): the element's log-prior term and its complete gradient
__device__ __forceinline__ void ga_z_prior(const RowsDev& R, double zq, double s_lane, double db, double& grad, double& lpz) {
  const double r = zq - R.z_np_mu;
  const double gx = -r * R.z_np_inv_var;
  lpz = -0.5 * r * r * R.z_np_inv_var - R.z_np_lognorm;
  grad = gx + s_lane * db;                                 // d/dz = prior + sigma_d * d/dbeta_d
}

// the hyper-parameter elements' local parts + their q' (lane e < 2D: element e; ONE wave does it for the launch -- with auxiliary
// workgroups, they do); their log-prior terms go into `lpg`
template <int D>
__device__ __forceinline__ void ga_hyper_local(const RowsDev& R, const ArenaDev& A, const Leaf& lf, double* def_loc, int par, bool leaf,
                                               int lane, double hval, double hph, double& lpg) {
  const int e = lane;
  const bool hact = e < 2 * D, is_mu = e < D;
  double gx, dxdq, dj, lpd;
  ga_def_local(R, is_mu, hval, gx, dxdq, dj, lpd);
  lpg += wave_sum(hact ? lpd : 0.0);
  if (hact) {
    const int dd = is_mu ? e : e - D;
    const int slot = (is_mu ? R.def_mu : R.def_sigma) + dd;
    double2* loc = reinterpret_cast<double2*>(def_loc + (int64_t)par * 4 * MAX_DEFERRED) + 2 * slot;
    loc[0] = make_double2(gx, dxdq);
    loc[1] = make_double2(dj, hph);
    if (leaf) A.Q[lf.d_o + (is_mu ? R.off_mu : R.off_sigma) + dd] = hval;
  }
}

// The tail wave of a chain in workgroup g: the group's D z elements (lane = coordinate), the hyper-parameter elements' local parts,
// leaf_post, the group's record and the block ticket -- on the chain's own arena, records `ga_part`, arrival counters `ga_ticket`
// and local parts `def_loc` (the three pointers come by reference: every caller keeps them in LDS, and each is read where it is
// used instead of being held in registers across leaf_post).  `lf`: the caller's resolve_leaf(io, A, j).  The five prologue
// values of the lane (ga_hyper, ga_z_state, ga_hyper_lanes) come by value; `mpf`: the merge operands the caller requested before
// its barrier, or nullptr.  s_info <- {last arriver of the block, m, last}.
// TREE: the launch is a tree leaf (the group kernels run nothing else); otherwise io.mode decides -- MODE_PLAIN writes io.grad
// and runs no leaf_post, MODE_SIMPLE builds no tree.
template <int D, bool TREE>
__device__ __forceinline__ void ga_tail_wave(const RowsDev& R, const ArenaDev& A, const EvalIO& io, double* const& ga_part, unsigned* const& ga_ticket,
                                             double* const& def_loc, const Leaf& lf, int g, int W, int j, int par, int d,
                                             const double (&s_acc)[GA_MAXW][2][D + 1], double* s_red, int* s_info,
                                             double hval, double hph, double zq, double zph, double s_lane, const MergePrefetch* mpf) {
  const int lane = threadIdx.x & (WAVE - 1);
  const bool leaf = TREE || io.mode != MODE_PLAIN;
  const bool tree = TREE || io.mode == MODE_TREE;
  const int dl = lane % D;
  const int iz = R.off_z + g * D + dl;
  double db = 0.0, lpg = 0.0;
  for (int ww = 0; ww < W; ++ww) { db += s_acc[ww][0][dl] + s_acc[ww][1][dl]; lpg += s_acc[ww][0][D] + s_acc[ww][1][D]; }
  const bool zact = lane < D;
  int idx[1] = {iz};
  bool act[1] = {zact};
  double grad[1] = {0.0}, ph[1] = {zph};
  {
    double lpz;
    ga_z_prior(R, zq, s_lane, db, grad[0], lpz);
    lpg += wave_sum(zact ? lpz : 0.0);
    if (zact) {
      if (leaf) { A.G[lf.d_o + iz] = grad[0]; A.Q[lf.d_o + iz] = zq; }
      else io.grad[iz] = grad[0];
    }
  }
  if (g == 0 && R.ga_naux == 0) ga_hyper_local<D>(R, A, lf, def_loc, par, leaf, lane, hval, hph, lpg);
  int m = 0; bool last = false;
  if (leaf) leaf_post<1>(A, lf, j, d, tree, idx, act, grad, ph, s_red, 1, m, last, tree ? mpf : nullptr, 0);   // (-> s_red[k]: the wave's own)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  // ---- this group's record, write-through ----
  double* rec = ga_part + (int64_t)g * PART_STRIDE;
  if (lane == 0) st_agent(rec + PART_LP, lpg);
  if (zact) { st_agent(rec + PART_DMU + lane, db); st_agent(rec + PART_DSG + lane, db * zq); }
  if (leaf) {
    for (int k = lane; k < NDOT; k += WAVE)
      if (dot_needed(k, m, last)) st_agent(rec + PART_DOT + k, s_red[k]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the record has left this CU before the ticket is taken

  // ---- ticket: the block's last arriver sums the block's records in group order ----
  const int blk = g / R.ga_bsz;
  const int cnt = min(R.G, (blk + 1) * R.ga_bsz) - blk * R.ga_bsz;
  unsigned old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(&ga_ticket[blk], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
  const int is_last = (int)old + 1 == cnt;
  if (is_last && lane == 0) __hip_atomic_store(&ga_ticket[blk], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (lane == 0) { s_info[0] = is_last; s_info[1] = m; s_info[2] = last ? 1 : 0; }
}

// slot q of the `nn` a record carries -> its place in the record: logp, d/dmu[D], d/dsigma[D], the dots of m merge levels, the six of `extend`
template <int D>
__device__ __forceinline__ int ga_need_slot(int q, int m) {
  if (q < 1) return PART_LP;
  if (q < 1 + D) return PART_DMU + (q - 1);
  if (q < 1 + 2 * D) return PART_DSG + (q - 1 - D);
  if (q < 1 + 2 * D + 1 + 6 * m) return PART_DOT + (q - 1 - 2 * D);
  return PART_DOT + DOT_TOP + (q - 1 - 2 * D - 1 - 6 * m);
}

// The last arriver's workgroup: block partial of a chain = sum of the block's records, chunks of 8 groups, chunks in order, into
// the chain's `ga_bpart` of launch parity `par` (every thread of the workgroup; s_info as ga_tail_wave left it; ends with the
// stores: a caller with several chains separates them with a barrier)
template <int D>
__device__ __forceinline__ void ga_block_partial(const RowsDev& R, const double* ga_part, double* ga_bpart, int par, int g, bool leaf,
                                                 const int* s_info, double (&s_cp)[GA_MAXCHUNK][PART_STRIDE]) {
  const int tid = threadIdx.x;
  const int m = s_info[1];
  const bool last = s_info[2] != 0;
  const int blk = g / R.ga_bsz, g0 = blk * R.ga_bsz;
  const int cnt = min(R.G, g0 + R.ga_bsz) - g0;
  const int nch = (cnt + 7) / 8;
  const int nn = 1 + 2 * D + (leaf ? 1 + 6 * m + (last ? 6 : 0) : 0);
  const int NT = (int)blockDim.x;
  for (int p = tid; p < nn * nch; p += NT) {
    const int c = p / nn, k = ga_need_slot<D>(p - c * nn, m);
    const int gg0 = c * 8, gcnt = min(8, cnt - gg0);
    const double* src = ga_part + (int64_t)(g0 + gg0) * PART_STRIDE + k;
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld_agent(src + (int64_t)min(u, gcnt - 1) * PART_STRIDE);
    double sum = 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += (u < gcnt) ? v[u] : 0.0;
    s_cp[c][k] = sum;
  }
  __syncthreads();
  double* bp = ga_bpart + ((int64_t)par * R.ga_nrec + blk) * PART_STRIDE;
  for (int q = tid; q < nn; q += NT) {
    const int k = ga_need_slot<D>(q, m);
    double sum = 0.0;
    for (int c = 0; c < nch; ++c) sum += s_cp[c][k];
    bp[k] = sum;
  }
}

// DX: stored columns of X per tile (D, or D - 1 = 7 when column 0 is identically 1; only with D = 8)
// PK: the seven stored columns come as packed 57-bit values (rows_pack.h; R.Xp and its own chunk offsets)
template <int D, int RPL, int DX = D, int PK = 0>
__global__ __launch_bounds__(64 * GA_MAXW, 4) void k_rows_ga(GaArgs a) {
  constexpr int SPAN = WAVE * RPL;
  static_assert(DX == D || (D == 8 && DX == 7), "only the intercept column of an 8-column model is elided");
  static_assert(!PK || (D == 8 && DX == 7 && RPL == 2), "packed tiles: seven stored columns, two rows per lane");
  typedef typename GaTileSel<DX, PK>::type Tile;
  constexpr int LOADS = PK ? 7 : DX + 1;   // loads per tile: the stored columns + y, or the seven planes of a packed tile
  const ModelDev& md = a.md;
  const ArenaDev& A = a.A;
  const EvalIO& io = a.io;
  const int j = a.j, rev = a.rev, fold = a.fold, par = a.par, d = a.d, max_depth = a.max_depth;
  const double Emax = a.Emax;
  HostStatus* const st = a.st;
  const RowsDev& R = md.lg;
  int b = (int)blockIdx.x;
  if (fold & GA_FOLD_CTL) {   // workgroup 0: control work, from the previous launch's block partials
    if (b == 0) { control_lean(md, A, a.cio, a.cj, a.cd, Emax, max_depth, st, a.cseq, lean_src(md, par ^ 1)); return; }
    --b;
  }
  const int g = b;
  // (the wave index is wave-uniform, but only `readfirstlane` tells the compiler: without it every tile address is per-lane
  // 64-bit VGPR arithmetic, and the streaming loop runs out of registers)
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6), W = (int)blockDim.x >> 6;
  Leaf lf; QView qv;
  const int aborted = load_aborted(io, A);
  resolve_leaf(io, A, j, lf, qv);
  const bool leaf = io.mode != MODE_PLAIN;
  __shared__ double s_acc[GA_MAXW][2][D + 1];   // [wave][first / second half of its tiles][d/dbeta, log-lik]
  __shared__ double s_red[NDOT];
  __shared__ double s_cp[GA_MAXCHUNK][PART_STRIDE];
  __shared__ int s_info[4];                      // {this workgroup is its block's last arriver, m, last}
  __shared__ double s_keep[5][WAVE];             // wave 0's per-lane prologue values the tail needs again (kept out of the stream's registers)
  __shared__ __attribute__((aligned(16))) char s_args[(sizeof(GaArgs) + 15) / 16 * 16];
  __shared__ __attribute__((aligned(16))) char s_auxprog[GA_AUX_PROG_LDS];   // auxiliary workgroups only (28 KB per workgroup in all: five per CU still fit)
  // workgroups behind the G groups: the auxiliary workgroups (rows_aux.h).  They take mu', sigma' of this leaf from the same
  // prologue arithmetic as everybody else and leave BEFORE any tile is requested: the call below may save registers around it,
  // and a register with a hand-counted load in flight must never be stored (tests/test_abi.py guards that).
  if (b >= R.G) {
    static_assert(GA_AUX_SCRATCH_DOUBLES(GA_MAXW) <= GA_MAXCHUNK * PART_STRIDE, "auxiliary scratch does not fit the chunk buffer");
    double hv, hp;
    ga_hyper<D>(R, qv, fold, lean_src(md, par ^ 1), lane, hv, hp);
    const int aux_id = b - R.G;
    // (LDS lent from the block reduce's chunk buffer, which only a block's last arriver uses)
    ga_aux<4>((const GaArgs*)__builtin_amdgcn_kernarg_segment_ptr(), aux_id, hv, hp, &s_cp[0][0], GA_MAXW, s_auxprog,
                R.ga_bpart + ((int64_t)par * R.ga_nrec + R.ga_nblk + aux_id) * PART_STRIDE, 1);
    return;
  }

  // ---- geometry of this wave's stream (no memory access when every group has the same number of rows) ----
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
  // The wave's tiles (its chunk) are streamed in two halves whose order alternates between launches (the tail of the previous
  // pass is still in the 256 MiB Infinity Cache); each half is summed in fixed tile order, wave-reduced and parked in its own
  // LDS slot, so the result does not depend on which half was streamed first.
  const int c0 = (int)((int64_t)w * T / W), c2 = (int)((int64_t)(w + 1) * T / W);   // this wave's tiles of the group: [c0, c2)
  const int n = c2 - c0;
  const int nA = (n + 1) / 2;                                   // tiles of the first half (chunk-local [0, nA)), second [nA, n)
  const int nsw = rev ? n - nA : nA;                            // position in the sequence where the second-streamed half starts
  constexpr int64_t TS = PK ? RP_TILE_DWORDS : (int64_t)DX * SPAN;   // doubles per tile (packed: dwords)
  auto local_at = [&](int i) { return rev ? (i < nsw ? nA + i : i - nsw) : i; };
  auto tile_at = [&](int i) { return cbase + (int64_t)local_at(i) * TS; };
  const int l_last = (c2 == T) ? n - 1 : -1;                    // chunk-local index of the group's last (zero-padded) tile, if it is here
  const int n_last = (int)(ng - (int64_t)(T - 1) * SPAN);     // its valid rows
  // two tiles in flight per wave; the first ones are requested before anything else, so HBM is busy during the prologue
  double xa[D][RPL], xb[D][RPL];
  uint32_t ya = 0, yb = 0;
  Tile ta, tb;
  // (a wave without tiles requests the chunk's first tile slot anyway: the layout keeps one tile of slack behind every chunk)
  uint64_t ea = 0, eb = 0;   // packed tiles: the exception ranges of the tiles in flight (scalar loads issued with the tiles)
  const int te0 = tg0 + c0;
  const GaPackOff vo{(uint32_t)lane * 16u, (uint32_t)lane * 4u};   // (packed tiles only)
  if constexpr (PK) {
    const int l1 = min(1, max(n - 1, 0));
    ga_issue8(R.Xp + tile_at(0), vo, ta);
    ga_issue8(R.Xp + tile_at(l1), vo, tb);
    ea = ga_exc_range(R.ga_pexc_idx, te0 + local_at(0));
    eb = ga_exc_range(R.ga_pexc_idx, te0 + local_at(l1));
  } else if constexpr (D == 8 && RPL == 2) {
    const uint32_t voff16 = (uint32_t)lane * 16u, voff2 = (uint32_t)lane * 2u;
    const int64_t o0 = tile_at(0), o1 = tile_at(min(1, max(n - 1, 0)));
    ga_issue8(R.Xt + o0, R.y + o0 / DX, voff16, voff2, ta);
    ga_issue8(R.Xt + o1, R.y + o1 / DX, voff16, voff2, tb);
  } else {
    ga_load<D, RPL>(R, tile_at(0), lane, xa, ya);
  }
  if (lane == 0) {
#pragma unroll
    for (int dd = 0; dd <= D; ++dd) { s_acc[w][0][dd] = 0.0; s_acc[w][1][dd] = 0.0; }
  }
  {
    const uint4* ka = (const uint4*)__builtin_amdgcn_kernarg_segment_ptr();
    for (int t = tid; t < (int)((sizeof(GaArgs) + 15) / 16); t += (int)blockDim.x) reinterpret_cast<uint4*>(s_args)[t] = ka[t];
  }
  __syncthreads();   // (every wave is still at the top of the kernel: this costs nothing, and the copy is readable from here on)

  // ---- prologue: mu', sigma' of this leaf (every wave), z' of this group ----
  double hval0, hph0;   // lane l: q' and p_half of hyper-parameter element l mod 2D
  ga_hyper<D>(R, qv, fold, lean_src(md, par ^ 1), lane, hval0, hph0);
  const int dl = lane % D;
  const int iz = R.off_z + g * D + dl;
  double beta[D];
  {
    double zq, zph, m_lane, s_lane;
    ga_z_state(qv, iz, zq, zph);
    ga_hyper_lanes<D>(R, hval0, dl, m_lane, s_lane);
    const double bl = fma(s_lane, zq, m_lane);
#pragma unroll
    for (int dd = 0; dd < D; ++dd) beta[dd] = readlane_d(bl, dd);
    if (w == 0) { s_keep[0][lane] = hval0; s_keep[1][lane] = hph0; s_keep[2][lane] = zq; s_keep[3][lane] = zph; s_keep[4][lane] = s_lane; }
  }
  if (aborted) return;   // (a workgroup that sees the flag takes no ticket: see the header)

  // ---- the stream ----
  {
    double acc[D], lp = 0.0;
#pragma unroll
    for (int dd = 0; dd < D; ++dd) acc[dd] = 0.0;
    int half = rev ? 1 : 0;   // which half of the wave's range the current accumulators belong to
    auto flush = [&]() {
#pragma unroll
      for (int dd = 0; dd < D; ++dd) {
        const double sum = wave_sum(acc[dd]);
        if (lane == 0) s_acc[w][half][dd] = sum;
        acc[dd] = 0.0;
      }
      const double sum = wave_sum(lp);
      if (lane == 0) s_acc[w][half][D] = sum;
      lp = 0.0;
      half ^= 1;
    };
#define GA_STAGE(X, Y, I)                                                                   \
    {                                                                                        \
      if ((I) == nsw) flush();                                                               \
      ga_tile<D, RPL>(X, Y, beta, local_at(I) == l_last ? n_last : SPAN, lane, acc, lp);     \
    }
    const int nm1 = n - 1;
    if constexpr (PK) {
      // packed tiles: the same two-deep stream with 7 loads per tile; a tile's exception range arrives with it
      const uint32_t ebase20 = R.ga_pack_ebase20;
      auto issue = [&](int i, Tile& t, uint64_t& er) {
        const int ii = min(i, nm1);
        ga_issue8(R.Xp + tile_at(ii), vo, t, acc, lp);
        er = ga_exc_range(R.ga_pexc_idx, te0 + local_at(ii));
      };
#define GA_PSTAGE(T, E, I)                                                                   \
      {                                                                                      \
        ga_wait8<LOADS>(T);                                                                  \
        if ((I) == nsw) flush();                                                             \
        double xx[8][2];                                                                     \
        ga_unpack(T, ebase20, xx);                                                           \
        const uint32_t yy = ga_ybits(T);                                                     \
        if ((uint32_t)((E) >> 32) != 0) ga_patch(R.ga_pexc, E, lane, xx);                    \
        ga_tile<8, 2>(xx, yy, beta, local_at(I) == l_last ? n_last : SPAN, lane, acc, lp);   \
      }
      for (int i = 0; i < n; i += 2) {
        GA_PSTAGE(ta, ea, i)
        if (i + 1 >= n) break;
        issue(i + 2, ta, ea);
        GA_PSTAGE(tb, eb, i + 1)
        issue(i + 3, tb, eb);
      }
      ga_wait8<0>(ta); ga_wait8<0>(tb);
#undef GA_PSTAGE
    } else if constexpr (D == 8 && RPL == 2) {
      // hand-counted loads: two tiles in flight per wave; the requests past the end re-read the wave's last tile (an L2 hit) so that
      // every stage has exactly 9 younger loads behind the tile it waits for
      const uint32_t voff16 = (uint32_t)lane * 16u, voff2 = (uint32_t)lane * 2u;
      auto issue = [&](int i, Tile& t) {
        const int64_t off = tile_at(min(i, nm1));
        ga_issue8(R.Xt + off, R.y + off / DX, voff16, voff2, t);
      };
#define GA_ASTAGE(T, I)                                                                      \
      {                                                                                      \
        ga_wait8<LOADS>(T);                                                                  \
        if ((I) == nsw) flush();                                                             \
        double xx[8][2];                                                                     \
        ga_unpack(T, xx);                                                                    \
        ga_tile<8, 2>(xx, ga_ybits(T), beta, local_at(I) == l_last ? n_last : SPAN, lane, acc, lp); \
      }
      for (int i = 0; i < n; i += 2) {
        GA_ASTAGE(ta, i)
        if (i + 1 >= n) break;
        issue(i + 2, ta);
        GA_ASTAGE(tb, i + 1)
        issue(i + 3, tb);
      }
      ga_wait8<0>(ta); ga_wait8<0>(tb);
#undef GA_ASTAGE
    } else {
      // compiler-counted loads.  The prefetch of tile i + 1 is UNCONDITIONAL (past the end it re-requests the wave's last tile):
      // a load inside an `if` makes hipcc drain every outstanding load (`s_waitcnt vmcnt(0)`) at the join.
      for (int i = 0; i < n; i += 2) {
        ga_load<D, RPL>(R, tile_at(min(i + 1, nm1)), lane, xb, yb);
        GA_STAGE(xa, ya, i)
        if (i + 1 >= n) break;
        ga_load<D, RPL>(R, tile_at(min(i + 2, nm1)), lane, xa, ya);
        GA_STAGE(xb, yb, i + 1)
      }
    }
#undef GA_STAGE
    if (n > 0) flush();
  }

  ga_tail<D>(*reinterpret_cast<const GaArgs*>(s_args), g, s_acc, s_red, s_cp, s_info, s_keep);
}

// Everything after the stream; `T` is the LDS copy of the kernel arguments.
template <int D>
__device__ __forceinline__ void ga_tail(const GaArgs& T, int g, double (&s_acc)[GA_MAXW][2][D + 1], double (&s_red)[NDOT],
                                        double (&s_cp)[GA_MAXCHUNK][PART_STRIDE], int (&s_info)[4], double (&s_keep)[5][WAVE]) {
  const ModelDev& md = T.md;
  const ArenaDev& A = T.A;
  const EvalIO& io = T.io;
  const RowsDev& R = md.lg;
  const int j = T.j;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid >> 6, W = (int)blockDim.x >> 6;
  Leaf lf; QView qv;
  resolve_leaf(io, A, j, lf, qv);
  const bool leaf = io.mode != MODE_PLAIN;
  const bool tree = io.mode == MODE_TREE;
  // the operands of the first merge levels belong to earlier leaves: wave 0 requests them as soon as its own stream is done,
  // before it waits for the other waves, so they are in flight during the combine
  const int dl = lane % D;
  const int iz = R.off_z + g * D + dl;
  MergePrefetch mpf;
  if (w == 0 && tree && !(R.ga_flags & GA_F_NOTAIL)) merge_prefetch(A, lf, j, iz, mpf);
  __syncthreads();
  if (R.ga_flags & GA_F_NOTAIL) return;

  if (w == 0)
    ga_tail_wave<D, false>(R, A, io, R.ga_part, R.ga_ticket, md.def_loc, lf, g, W, j, T.par, T.d, s_acc, s_red, s_info,
                           s_keep[0][lane], s_keep[1][lane], s_keep[2][lane], s_keep[3][lane], s_keep[4][lane], &mpf);
  __syncthreads();
  if (!s_info[0]) return;
  ga_block_partial<D>(R, R.ga_part, R.ga_bpart, T.par, g, leaf, s_info, s_cp);
}

// A leaf whose wave sums were evaluated ahead (edge pairing): the launch of `k_rows_ga` without its stream.  No tile is requested;
// the prologue is the one above on the same source state (only the tail wave needs its values: nobody forms beta_g), every
// workgroup copies its ring entry into `s_acc`, and `ga_tail` runs as it stands -- the tree sees today's code on today's operands.
// `ring`: this leaf's entry, [G][GA_MAXW][2][D + 1].  Models with auxiliary workgroups are not eligible (engine.hip).
template <int D>
__global__ __launch_bounds__(64 * GA_MAXW, 4) void k_rows_ga_replay(GaArgs a, const double* __restrict__ ring) {
  const ModelDev& md = a.md;
  const ArenaDev& A = a.A;
  const EvalIO& io = a.io;
  const int fold = a.fold, par = a.par;
  const RowsDev& R = md.lg;
  int b = (int)blockIdx.x;
  if (fold & GA_FOLD_CTL) {   // workgroup 0: control work, from the previous launch's block partials
    if (b == 0) { control_lean(md, A, a.cio, a.cj, a.cd, a.Emax, a.max_depth, a.st, a.cseq, lean_src(md, par ^ 1)); return; }
    --b;
  }
  const int g = b;
  if (g >= R.G) return;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = __builtin_amdgcn_readfirstlane(tid >> 6);
  Leaf lf; QView qv;
  const int aborted = load_aborted(io, A);
  resolve_leaf(io, A, a.j, lf, qv);
  __shared__ double s_acc[GA_MAXW][2][D + 1];
  __shared__ double s_red[NDOT];
  __shared__ double s_cp[GA_MAXCHUNK][PART_STRIDE];
  __shared__ int s_info[4];
  __shared__ double s_keep[5][WAVE];
  __shared__ __attribute__((aligned(16))) char s_args[(sizeof(GaArgs) + 15) / 16 * 16];
  constexpr int NR = GA_RING_DOUBLES(D);
  static_assert(NR <= 2 * WAVE, "two doubles of a ring entry per thread at most");
  const double rv0 = ring[(int64_t)g * NR + min(tid, NR - 1)], rv1 = ring[(int64_t)g * NR + min(tid + WAVE, NR - 1)];   // (requested first)
  {
    const uint4* ka = (const uint4*)__builtin_amdgcn_kernarg_segment_ptr();
    for (int t = tid; t < (int)((sizeof(GaArgs) + 15) / 16); t += (int)blockDim.x) reinterpret_cast<uint4*>(s_args)[t] = ka[t];
  }
  __syncthreads();   // (the copy is readable from here on)
  if (w == 0) {
    double hval0, hph0, zq, zph, m_lane, s_lane;
    ga_hyper<D>(R, qv, fold, lean_src(md, par ^ 1), lane, hval0, hph0);
    const int dl = lane % D;
    ga_z_state(qv, R.off_z + g * D + dl, zq, zph);
    ga_hyper_lanes<D>(R, hval0, dl, m_lane, s_lane);
    s_keep[0][lane] = hval0; s_keep[1][lane] = hph0; s_keep[2][lane] = zq; s_keep[3][lane] = zph; s_keep[4][lane] = s_lane;
  }
  if (aborted) return;   // (no ticket, as a streamed leaf)
  if (tid < WAVE) {   // (a workgroup has at least one wave)
    (&s_acc[0][0][0])[tid] = rv0;
    if (tid + WAVE < NR) (&s_acc[0][0][0])[tid + WAVE] = rv1;
  }
  ga_tail<D>(*reinterpret_cast<const GaArgs*>(s_args), g, s_acc, s_red, s_cp, s_info, s_keep);
}
