// A stand-alone host program around pymc_amd/csrc/prior.h (tests/test_prior_host.py builds it with the system compiler, warnings as
// errors, address and undefined-behaviour sanitizers where they link).  Standard input, one request after another:
//   draw dist a1 a2 a3 transform lower upper seed index s0 ns i0 ni   -> ns * ni prior variates of variable `index`, pushed through
//                                                                        the forward transform, draw-major, as hex floats / inf / nan
//   dirichlet K alpha_0.. seed index s0 ns                           -> ns * (K - 1) simplex-transformed values of Dirichlet draws
//   forward transform lower upper x                                  -> the forward transform of x
//   counters index s i t_last                                        -> for t = 0 .. t_last the four counter words of the prior
//                                                                        variate, then those of observed node (kind, index), kind 0 .. 3
// Integers are decimal or 0x-hex, doubles as strtod reads them.  Exit status 2: malformed input; 4: a refused family or an index or
// draw number that does not fit the counter.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "prior.h"

static bool next_token(std::string& tok) {
  tok.clear();
  int ch;
  while ((ch = std::getchar()) != EOF && (ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r')) {}
  if (ch == EOF) return false;
  do { tok.push_back((char)ch); } while ((ch = std::getchar()) != EOF && ch != ' ' && ch != '\n' && ch != '\t' && ch != '\r');
  return true;
}

static double need_double() {
  std::string tok;
  if (!next_token(tok)) std::exit(2);
  char* end = nullptr;
  const double v = std::strtod(tok.c_str(), &end);
  if (end == tok.c_str() || *end != '\0') std::exit(2);
  return v;
}

static uint64_t need_u64() {
  std::string tok;
  if (!next_token(tok) || tok[0] == '-') std::exit(2);
  char* end = nullptr;
  const unsigned long long v = std::strtoull(tok.c_str(), &end, 0);
  if (end == tok.c_str() || *end != '\0') std::exit(2);
  return (uint64_t)v;
}

static uint32_t need_tag() {
  const uint64_t index = need_u64();
  uint32_t tag = 0;
  if (index > 0x7fffffff || !prior_tag((int32_t)index, &tag)) std::exit(4);
  return tag;
}

static void put(double v) { std::printf("%a\n", v); }

int main() {
  std::string what;
  while (next_token(what)) {
    if (what == "draw") {
      const int dist = (int)need_u64();
      const double a1 = need_double(), a2 = need_double(), a3 = need_double();
      const int transform = (int)need_u64();
      const double lower = need_double(), upper = need_double();
      const uint64_t seed = need_u64();
      const uint32_t tag = need_tag();
      const uint64_t s0 = need_u64(), ns = need_u64(), i0 = need_u64(), ni = need_u64();
      if (!prior_family_ok(dist) || s0 + ns > (1ull << 32)) return 4;
      for (uint64_t s = s0; s < s0 + ns; ++s)
        for (uint64_t i = i0; i < i0 + ni; ++i)
          put(prior_forward(transform, lower, upper, pp_draw(dist, 0.0, a1, a2, a3, pp_key(seed), prior_ctr((int64_t)i, (uint32_t)s, tag))));
    } else if (what == "dirichlet") {
      const uint64_t K = need_u64();
      if (K < 3 || K > PRIOR_MAXK) return 2;
      std::vector<double> alpha((size_t)K), y((size_t)K);
      for (double& v : alpha) v = need_double();
      const uint64_t seed = need_u64();
      const uint32_t tag = need_tag();
      const uint64_t s0 = need_u64(), ns = need_u64();
      if (s0 + ns > (1ull << 32)) return 4;
      for (uint64_t s = s0; s < s0 + ns; ++s) {
        prior_dirichlet((int)K, alpha.data(), pp_key(seed), (uint32_t)s, tag, y.data(), nullptr);
        for (uint64_t k = 0; k + 1 < K; ++k) put(y[(size_t)k]);
      }
    } else if (what == "forward") {
      const int transform = (int)need_u64();
      const double lower = need_double(), upper = need_double(), x = need_double();
      put(prior_forward(transform, lower, upper, x));
    } else if (what == "counters") {
      const uint64_t index = need_u64(), s = need_u64(), i = need_u64(), t_last = need_u64();
      uint32_t tag = 0;
      if (index > 0x3fff || !prior_tag((int32_t)index, &tag) || t_last > 0xffff) return 4;
      for (uint32_t t = 0; t <= (uint32_t)t_last; ++t) {
        const PPCtr p = prior_ctr((int64_t)i, (uint32_t)s, tag);
        std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", p.c0, p.c1, p.c2, p.c3 | t);
        for (int32_t kind = 0; kind < 4; ++kind) {
          uint32_t ntag = 0;
          if (!pp_tag(kind, (int32_t)index, &ntag)) return 4;
          const PPCtr c = pp_ctr((int64_t)i, (uint32_t)s, ntag);
          std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", c.c0, c.c1, c.c2, c.c3 | t);
        }
      }
    } else
      return 2;
  }
  return 0;
}
