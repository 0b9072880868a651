// Stand-alone checks of pymc_amd/csrc/rows_pack.h (compiled and run by tests/test_rows_pack_cpu.py).
// usage: rows_pack_check <section>   -- prints "ok" and exits 0, or says what differs and exits 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "rows_pack.h"

static const int ELO = 1023 - 13;   // the window [-13, 3)

static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

struct Tile {
  std::vector<double> cols = std::vector<double>((size_t)RP_COLS * RP_ROWS, 0.0);
  std::vector<int8_t> y = std::vector<int8_t>(RP_ROWS, 0);
  double& at(int lane, int slot) { return cols[(size_t)(slot >> 1) * RP_ROWS + 2 * lane + (slot & 1)]; }
};

static Tile normal_tile(unsigned seed) {
  Tile t;
  std::mt19937_64 rng(seed);
  std::normal_distribution<double> nd(0.0, 1.0);
  for (auto& v : t.cols) v = nd(rng);
  for (auto& v : t.y) v = (int8_t)(rng() & 1);
  return t;
}

// pack -> unpack: every valid row bit-identical, padding decodes to the finite placeholder with y = 0; the number of
// exceptions is `want_exc` (< 0: not checked)
static bool roundtrip(Tile& t, int nvalid, long want_exc, const char* what) {
  std::vector<uint32_t> packed(RP_TILE_DWORDS, 0xdeadbeefu);
  std::vector<RpExc> exc;
  rp_pack_tile(t.cols.data(), t.y.data(), nvalid, ELO, 5u, packed.data(), exc);
  std::vector<double> cols((size_t)RP_COLS * RP_ROWS, -1.0);
  std::vector<int8_t> y(RP_ROWS, 7);
  rp_unpack_tile(packed.data(), ELO, exc.data(), exc.size(), 5u, cols.data(), y.data());
  const double placeholder = std::ldexp(1.0, ELO - 1023);
  for (int c = 0; c < RP_COLS; ++c)
    for (int r = 0; r < RP_ROWS; ++r) {
      const double want = r < nvalid ? t.cols[(size_t)c * RP_ROWS + r] : placeholder;
      const double got = cols[(size_t)c * RP_ROWS + r];
      if (bits_of(want) != bits_of(got)) {
        printf("%s: column %d row %d: %016llx != %016llx\n", what, c, r, (unsigned long long)bits_of(got), (unsigned long long)bits_of(want));
        return false;
      }
    }
  for (int r = 0; r < RP_ROWS; ++r)
    if (y[r] != (r < nvalid ? t.y[r] : 0)) { printf("%s: y of row %d\n", what, r); return false; }
  // the packed slot of an exception holds a finite in-window value (what the kernel decodes before the patch)
  std::vector<double> raw((size_t)RP_COLS * RP_ROWS);
  rp_unpack_tile(packed.data(), ELO, nullptr, 0, 5u, raw.data(), y.data());
  for (double v : raw)
    if (!std::isfinite(v) || !rp_in_window(bits_of(v), ELO)) { printf("%s: a packed slot decodes outside the window\n", what); return false; }
  for (const RpExc& e : exc)
    if (e.tile != 5u || (e.lane_slot & 0xff) >= RP_LANES || (e.lane_slot >> 8) >= RP_SLOTS) { printf("%s: malformed exception\n", what); return false; }
  if (want_exc >= 0 && (long)exc.size() != want_exc) { printf("%s: %zu exceptions, expected %ld\n", what, exc.size(), want_exc); return false; }
  return true;
}

static bool section_roundtrip() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double lo_edge = std::ldexp(1.0, -13), hi_edge = std::ldexp(1.0, 3);
  bool ok = true;
  {   // N(0,1): the exceptions are exactly the values outside the window
    Tile t = normal_tile(1);
    long n = 0;
    for (double v : t.cols) n += !rp_in_window(bits_of(v), ELO);
    ok = ok && roundtrip(t, RP_ROWS, n, "normal");
  }
  {   // both window edges, both signs
    Tile t = normal_tile(2);
    long n = 0;
    for (double v : t.cols) n += !rp_in_window(bits_of(v), ELO);
    const double vals[6] = {lo_edge, -lo_edge, std::nextafter(hi_edge, 0.0), -std::nextafter(hi_edge, 0.0), hi_edge, -hi_edge};
    for (int k = 0; k < 6; ++k) { double& x = t.at(7 + k, (3 * k) % RP_SLOTS); n -= !rp_in_window(bits_of(x), ELO); x = vals[k]; }
    ok = ok && roundtrip(t, RP_ROWS, n + 2, "edges");   // (2^(lo+16) itself is outside)
    Tile u = normal_tile(3);
    u.at(9, 4) = std::nextafter(lo_edge, 0.0);          // the largest value below the window
    ok = ok && roundtrip(u, RP_ROWS, -1, "below");
  }
  {   // the special values, in lane 0 and lane 63, slot 0 and slot 13, several in one lane
    Tile t = normal_tile(4);
    long n = 0;
    for (double& v : t.cols) if (!rp_in_window(bits_of(v), ELO)) v = 1.0;
    const double sp[8] = {0.0, -0.0, 4.9406564584124654e-324, 1e300, -1e300, nan, inf, -inf};
    for (int k = 0; k < 8; ++k) { t.at(0, k) = sp[k]; ++n; }            // eight in lane 0, slot 0 among them
    t.at(0, 13) = nan; ++n;
    t.at(63, 0) = -inf; t.at(63, 13) = 0.0; n += 2;
    t.at(31, 6) = 1e300; t.at(31, 7) = -0.0; n += 2;
    ok = ok && roundtrip(t, RP_ROWS, n, "specials");
  }
  for (int nvalid : {1, 2, 127}) {   // a group's last tile
    Tile t = normal_tile(10 + nvalid);
    t.at(0, 0) = 0.0;                 // row 0: an exception in the only valid row
    t.at(63, 1) = inf; t.at(63, 0) = -0.0;   // rows 127 (padding unless nvalid = 128) and 126
    long n = 0;
    for (int c = 0; c < RP_COLS; ++c)
      for (int r = 0; r < nvalid; ++r) n += !rp_in_window(bits_of(t.cols[(size_t)c * RP_ROWS + r]), ELO);
    ok = ok && roundtrip(t, nvalid, n, ("last tile " + std::to_string(nvalid)).c_str());
  }
  return ok;
}

static void normal_matrix(std::vector<double>& X, std::vector<int8_t>& y, int64_t N, unsigned seed) {
  X.resize((size_t)N * 8); y.resize((size_t)N);
  std::mt19937_64 rng(seed);
  std::normal_distribution<double> nd(0.0, 1.0);
  for (int64_t i = 0; i < N; ++i) {
    X[(size_t)i * 8] = 1.0;
    for (int d = 1; d < 8; ++d) X[(size_t)i * 8 + d] = nd(rng);
    y[(size_t)i] = (int8_t)(rng() & 1);
  }
}

// 16 M standard normal values: [-13, 3) loses P(|x| < 2^-13) = 9.7e-5; its neighbours [-14, 2) and [-12, 4) lose 1.1e-4 and 1.9e-4
// -- 230 and 1500 values more at this size, against a standard deviation of about 40
static bool section_window() {
  std::vector<double> X; std::vector<int8_t> y;
  normal_matrix(X, y, 2300000, 99);
  const RpPlan p = rp_plan(X.data(), 2300000, 8, 1, y.data());
  const double share = (double)p.n_exc / (double)p.n_values;
  printf("window [%d, %d), share outside %.3e\n", p.elo - 1023, p.elo - 1023 + RP_WINDOW, share);
  return p.elo == ELO && p.eligible && p.y01 && share > 5e-5 && share < 1.5e-4;
}

static bool section_eligible() {
  std::vector<double> X; std::vector<int8_t> y;
  normal_matrix(X, y, 20000, 7);
  bool ok = rp_plan(X.data(), 20000, 8, 1, y.data()).eligible;
  std::vector<double> Xd = X;
  for (int64_t i = 0; i < 20000; ++i) Xd[(size_t)i * 8 + 3] = (double)(i % 3 == 0);   // a 0/1 dummy column: every 0 is an exception
  const RpPlan pd = rp_plan(Xd.data(), 20000, 8, 1, y.data());
  ok = ok && !pd.eligible && pd.y01;
  std::vector<int8_t> y2 = y;
  y2[123] = 2;                                                                       // y beyond 0 / 1
  const RpPlan py = rp_plan(X.data(), 20000, 8, 1, y2.data());
  ok = ok && !py.eligible && !py.y01;
  return ok;
}

int main(int argc, char** argv) {
  const std::string s = argc > 1 ? argv[1] : "";
  bool ok = false;
  if (s == "roundtrip") ok = section_roundtrip();
  else if (s == "window") ok = section_window();
  else if (s == "eligible") ok = section_eligible();
  else { printf("unknown section '%s'\n", s.c_str()); return 2; }
  printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
