// Lossless 57-bit packing of the X tiles the group-aligned row pass streams (rows_ga_kernel.h, D = 8 with the intercept column
// elided, two rows per lane): 6400 B per 128-row tile instead of 7296 B.
//
// A stored value is an fp64: sign, 11 exponent bits, 52 mantissa bits.  For standardised covariates the exponent carries about
// 3 bits of information: all but ~1e-4 of the values have floor(log2|x|) inside ONE window of 16 binades.  Inside the window
//   low dword   = the fp64's low dword, as stored                                                     (32 bits)
//   high field  = sign (bit 24) | exponent - window's lowest biased exponent (bits 23..20) | mantissa bits 51..32 (bits 19..0)
//                                                                                                      (25 bits)
// and the high dword is rebuilt as  sign << 31 | ((field & 0xffffff) + (ebase << 20)).  y (0 / 1) is one bit.  A lane of a tile
// owns 2 rows x 7 columns = 14 SLOTS (slot = 2 column + row): 14 x 57 + 2 = 800 bits = 100 B per lane.
//
// Values outside the window (+-0, denormals, infinities, NaNs and the few large / tiny ones) are EXCEPTIONS: their packed slot
// holds the finite in-window pattern 0 (the value 2^lo), the raw 8 bytes travel in a side list and are patched in after the decode.
// The padded rows of a group's last tile hold the same pattern (they are masked, but fma(0, x, acc) needs a finite x).
//
// Tile layout: a lane owns 25 dwords -- dwords 0..13 the low dwords of its slots, dwords 14..24 its 352-bit string (little-endian:
// field i at bit 25 i, y of row 0 at bit 350, y of row 1 at bit 351).  They are lane-transposed into seven planes so that every
// wave load reads ONE contiguous block (lane l reads at plane + l * width):
//   plane k = 0..5 at byte 1024 k: dwords 4k .. 4k+3, 16 B per lane (dwordx4)
//   plane 6 at byte 6144:          dword 24,           4 B per lane (dword; 256 B)
// (All planes but the last are 128-bit loads, the register class of the raw tile's loads: a 96-bit plane made the register
// allocator move a tile between two register triples inside the streaming loop, while its load was in flight.)
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RP_HD __host__ __device__ __forceinline__
#else
#define RP_HD inline
#endif

#define RP_LANES 64
#define RP_ROWS 128             // rows per tile: two per lane
#define RP_COLS 7               // stored columns
#define RP_SLOTS 14             // per lane: slot = 2 * column + row
#define RP_FIELD_BITS 25
#define RP_WINDOW 16            // binades
#define RP_HI_DWORDS 11         // 352 bits per lane
#define RP_TILE_BYTES 6400
#define RP_TILE_DWORDS 1600
#define RP_LANE_DWORDS 25       // 14 low dwords + the 11 dwords of the string
#define RP_MAX_EXC_SHARE 1e-3   // eligibility: at most this share of the stored values may be exceptions

// high dword of a value from its 25-bit field (bits above 24 of `f` are ignored); ebase20 = lowest biased exponent of the window << 20
RP_HD uint32_t rp_decode_hi(uint32_t f, uint32_t ebase20) { return ((f << 7) & 0x80000000u) | ((f & 0xffffffu) + ebase20); }

// field i of a lane's 352-bit string `h` (11 dwords); only bits 0..24 of the result are meaningful
RP_HD uint32_t rp_field(const uint32_t* h, int i) {
  const int q = (RP_FIELD_BITS * i) >> 5, r = (RP_FIELD_BITS * i) & 31;
  if (r + RP_FIELD_BITS <= 32) return h[q] >> r;
  return (h[q] >> r) | (h[q + 1] << (32 - r));
}

// position of dword d of lane `lane` in the tile (in dwords)
RP_HD int rp_dword_at(int lane, int d) { return d < 24 ? (d >> 2) * 256 + lane * 4 + (d & 3) : 1536 + lane; }

// one exception: the raw bits of the value at (chunk-local tile, lane, slot)
// (`tile` serves the host unpacker below, which is handed a flat list; the kernel never reads it: it finds a tile's entries
// through the per-tile range table, RowsDev::ga_pexc_idx.  It stays in the device copy so that an entry is one 16 B scalar load.)
struct alignas(16) RpExc { uint32_t tile, lane_slot /* lane | slot << 8 */, lo, hi; };

// ---- host side: plan, packer, unpacker ----
#include <vector>

// value with biased exponent e is inside the window starting at biased exponent elo
inline bool rp_in_window(uint64_t bits, int elo) {
  const int e = (int)((bits >> 52) & 0x7ff);
  return e >= elo && e < elo + RP_WINDOW;
}

// the 16-binade window with the fewest values outside it; hist[e] = number of values with biased exponent e (0 = zeros and
// denormals, 2047 = infinities and NaNs: never inside).  Returns the window's lowest biased exponent (ties: the lowest one).
inline int rp_choose_window(const uint64_t (&hist)[2048], uint64_t* n_outside) {
  uint64_t total = 0, in = 0, best_in = 0;
  for (int e = 0; e < 2048; ++e) total += hist[e];
  int best = 1;
  for (int e = 1; e < 1 + RP_WINDOW; ++e) in += hist[e];
  best_in = in;
  for (int elo = 2; elo + RP_WINDOW <= 2047; ++elo) {
    in += hist[elo + RP_WINDOW - 1]; in -= hist[elo - 1];
    if (in > best_in) { best_in = in; best = elo; }
  }
  if (n_outside) *n_outside = total - best_in;
  return best;
}

struct RpPlan {
  int elo;               // lowest biased exponent of the window (window = binades [elo - 1023, elo - 1023 + 16))
  uint64_t n_values, n_exc;
  bool y01, eligible;
};

// Scan a row-major matrix X[N][D], columns first_col .. D-1 stored, and y[N]: window, exception count, eligibility of the DATA
// (the caller adds the structural conditions: D = 8 with the intercept elided, two rows per lane, the single-chain pass).
inline RpPlan rp_plan(const double* X, int64_t N, int D, int first_col, const int8_t* y) {
  uint64_t hist[2048] = {0};
  RpPlan p; p.y01 = true;
  for (int64_t i = 0; i < N; ++i) {
    for (int d = first_col; d < D; ++d) {
      uint64_t b; memcpy(&b, &X[i * D + d], 8);
      hist[(b >> 52) & 0x7ff]++;
    }
    p.y01 = p.y01 && (y[i] == 0 || y[i] == 1);
  }
  p.n_values = (uint64_t)N * (uint64_t)(D - first_col);
  p.elo = rp_choose_window(hist, &p.n_exc);
  p.eligible = p.y01 && p.n_values > 0 && (double)p.n_exc <= RP_MAX_EXC_SHARE * (double)p.n_values;
  return p;
}

// Pack one tile.  cols: [7][128] doubles (column c, row r at cols[c * 128 + r]); y: [128]; rows >= nvalid are padding.
// out: 1600 dwords.  Exceptions are appended to `exc` with `tile` as given.
inline void rp_pack_tile(const double* cols, const int8_t* y, int nvalid, int elo, uint32_t tile, uint32_t* out, std::vector<RpExc>& exc) {
  memset(out, 0, RP_TILE_BYTES);
  for (int lane = 0; lane < RP_LANES; ++lane) {
    uint32_t h[RP_HI_DWORDS + 1] = {0};
    for (int s = 0; s < RP_SLOTS; ++s) {
      const int c = s >> 1, r = 2 * lane + (s & 1);
      uint32_t lo = 0, f = 0;   // the pattern of padding and exceptions: 2^(elo - 1023)
      if (r < nvalid) {
        uint64_t b; memcpy(&b, &cols[c * RP_ROWS + r], 8);
        if (rp_in_window(b, elo)) {
          lo = (uint32_t)b;
          const uint32_t hi = (uint32_t)(b >> 32);
          f = ((hi >> 31) << 24) | ((((hi >> 20) & 0x7ff) - (uint32_t)elo) << 20) | (hi & 0xfffffu);
        } else exc.push_back(RpExc{tile, (uint32_t)lane | ((uint32_t)s << 8), (uint32_t)b, (uint32_t)(b >> 32)});
      }
      out[rp_dword_at(lane, s)] = lo;
      const int q = (RP_FIELD_BITS * s) >> 5, sh = (RP_FIELD_BITS * s) & 31;
      h[q] |= f << sh;
      if (sh + RP_FIELD_BITS > 32) h[q + 1] |= f >> (32 - sh);
    }
    for (int k = 0; k < 2; ++k)
      if (2 * lane + k < nvalid && y[2 * lane + k]) h[10] |= 1u << (30 + k);
    for (int q = 0; q < RP_HI_DWORDS; ++q) out[rp_dword_at(lane, RP_SLOTS + q)] = h[q];
  }
}

// The inverse, for tests: decodes every slot (exceptions of this tile applied from exc[0 .. n_exc)) into cols / y.
inline void rp_unpack_tile(const uint32_t* in, int elo, const RpExc* exc, size_t n_exc, uint32_t tile, double* cols, int8_t* y) {
  const uint32_t ebase20 = (uint32_t)elo << 20;
  for (int lane = 0; lane < RP_LANES; ++lane) {
    uint32_t h[RP_HI_DWORDS];
    for (int q = 0; q < RP_HI_DWORDS; ++q) h[q] = in[rp_dword_at(lane, RP_SLOTS + q)];
    for (int s = 0; s < RP_SLOTS; ++s) {
      const uint32_t lo = in[rp_dword_at(lane, s)];
      const uint64_t b = ((uint64_t)rp_decode_hi(rp_field(h, s), ebase20) << 32) | lo;
      memcpy(&cols[(s >> 1) * RP_ROWS + 2 * lane + (s & 1)], &b, 8);
    }
    y[2 * lane] = (int8_t)((h[10] >> 30) & 1u);
    y[2 * lane + 1] = (int8_t)(h[10] >> 31);
  }
  for (size_t k = 0; k < n_exc; ++k) {
    if (exc[k].tile != tile) continue;
    const int lane = (int)(exc[k].lane_slot & 0xff), s = (int)(exc[k].lane_slot >> 8);
    const uint64_t b = ((uint64_t)exc[k].hi << 32) | exc[k].lo;
    memcpy(&cols[(s >> 1) * RP_ROWS + 2 * lane + (s & 1)], &b, 8);
  }
}
