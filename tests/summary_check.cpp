// A stand-alone host program around pymc_amd/csrc/summary.h (tests/test_summary_host.py builds it with the system compiler, warnings
// as errors, address and undefined-behaviour sanitizers where they link).  Standard input, one request after another, every token
// as strtod reads it (hex floats, nan, inf, -inf):
//   1 c n v_0 ... v_{c n - 1}     ESS of c chains of n draws (chain-major): chain means, centred lagged products, sm_ess
//   2 c n v_0 ... v_{c n - 1}     split R-hat formula of the same layout: W, B, sm_rhat
//   3 S prob v_0 ... v_{S-1}      HDI of the values (sorted here): lo hi
//   4 S q v_0 ... v_{S-1}         numpy.quantile(v, q) of the values (sorted here)
//   5 p                           ndtri(p)
// Standard output per request: its one or two results as hex floats.  Exit status 2: malformed input; 3: the strided form of the
// HDI scan (what a workgroup runs) disagreed with the sequential one.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "summary.h"

static bool next_token(std::string& tok) {
  tok.clear();
  int ch;
  while ((ch = std::getchar()) != EOF && (ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r')) {}
  if (ch == EOF) return false;
  do { tok.push_back((char)ch); } while ((ch = std::getchar()) != EOF && ch != ' ' && ch != '\n' && ch != '\t' && ch != '\r');
  return true;
}

static bool next_double(double& v) {
  std::string tok;
  if (!next_token(tok)) return false;
  char* end = nullptr;
  v = std::strtod(tok.c_str(), &end);
  if (end == tok.c_str() || *end != '\0') std::exit(2);
  return true;
}

static bool read_values(std::vector<double>& v, int64_t count) {
  if (count < 0 || count > (1 << 24)) return false;
  v.resize((size_t)count);
  for (auto& e : v)
    if (!next_double(e)) return false;
  return true;
}

int main() {
  double op_in;
  while (next_double(op_in)) {
    const int op = (int)op_in;
    std::vector<double> v;
    if (op == 1 || op == 2) {
      double c_in, n_in;
      if (!next_double(c_in) || !next_double(n_in)) return 2;
      const int64_t c = (int64_t)c_in, n = (int64_t)n_in;
      if (c < 1 || n < 1 || !read_values(v, c * n)) return 2;
      std::vector<double> cm((size_t)c);
      double ss = 0.0, gm = 0.0, vm = 0.0;
      for (int64_t k = 0; k < c; ++k) {
        double a = 0.0;
        for (int64_t i = 0; i < n; ++i) a += v[(size_t)(k * n + i)];
        cm[(size_t)k] = a / (double)n;
        for (int64_t i = 0; i < n; ++i) { double& e = v[(size_t)(k * n + i)]; e -= cm[(size_t)k]; ss += e * e; }
        gm += cm[(size_t)k];
      }
      gm /= (double)c;
      for (int64_t k = 0; k < c; ++k) vm += (cm[(size_t)k] - gm) * (cm[(size_t)k] - gm);
      if (c > 1) vm /= (double)(c - 1);
      if (op == 2) {
        std::printf("%a\n", sm_rhat(n, ss / (double)(n - 1) / (double)c, (double)n * vm));
        continue;
      }
      const double tot = (double)n * (double)c;
      const double e = sm_ess(c, n, ss / tot, vm, [&](int64_t t) {
        double a = 0.0;
        for (int64_t k = 0; k < c; ++k)
          for (int64_t i = 0; i + t < n; ++i) a += v[(size_t)(k * n + i)] * v[(size_t)(k * n + i + t)];
        return a / tot;
      });
      std::printf("%a\n", e);
    } else if (op == 3 || op == 4) {
      double s_in, q;
      if (!next_double(s_in) || !next_double(q)) return 2;
      const int64_t S = (int64_t)s_in;
      if (S < 1 || !read_values(v, S)) return 2;
      std::sort(v.begin(), v.end());
      if (op == 4) { std::printf("%a\n", sm_quantile(v.data(), S, q)); continue; }
      const int64_t k = sm_hdi_k(q, S);
      if (S - k < 1) { std::printf("nan nan\n"); continue; }
      double bw, w; int64_t bi, i;
      sm_hdi_scan(v.data(), S, k, 0, 1, bw, bi);
      double cw = INFINITY; int64_t ci = -1;
      for (int64_t start = 6; start >= 0; --start) {   // seven interleaved ranges, combined from the last to the first
        sm_hdi_scan(v.data(), S, k, start, 7, w, i);
        if (sm_hdi_better(w, i, cw, ci)) { cw = w; ci = i; }
      }
      if (ci != bi) return 3;
      std::printf("%a %a\n", v[(size_t)bi], v[(size_t)(bi + k)]);
    } else if (op == 5) {
      double p;
      if (!next_double(p)) return 2;
      std::printf("%a\n", sm_ndtri(p));
    } else
      return 2;
  }
  return 0;
}
