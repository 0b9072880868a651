// A stand-alone host program around pymc_amd/csrc/psis.h (tests/test_psis_host.py builds it with the system compiler, warnings as
// errors, address and undefined-behaviour sanitizers where they link).  Standard input, one case after another:
//   S reff stride column v_0 ... v_{S-1}      (values as strtod reads them: hex floats, nan, inf, -inf)
// The values are folded draw by draw into column `column` of a [K1][stride] block exactly as k_psis_fold folds them, then finished.
// Standard output per case: khat elpd_loo_i m_rest r_rest as hex floats.  Exit status 2: malformed input; 3: a neighbouring column
// of the block was written.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "psis.h"

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

int main() {
  const double SENTINEL = -12345.678;
  double s_in;
  while (next_double(s_in)) {
    double reff, stride_in, col_in;
    if (!next_double(reff) || !next_double(stride_in) || !next_double(col_in)) return 2;
    const int64_t S = (int64_t)s_in, stride = (int64_t)stride_in, col = (int64_t)col_in;
    if (S < 2 || !(reff > 0.0) || stride < 1 || col < 0 || col >= stride) return 2;
    const int64_t K1 = psis_tail_len(S, reff) + 1;
    if (K1 > PSIS_K1_MAX) return 2;
    std::vector<double> keep((size_t)(K1 * stride), SENTINEL);
    for (int64_t j = 0; j < K1; ++j) keep[(size_t)(j * stride + col)] = INFINITY;
    double m_rest = -INFINITY, r_rest = 0.0;
    for (int64_t s = 0; s < S; ++s) {
      double v;
      if (!next_double(v)) return 2;
      if (!(v < keep[(size_t)((K1 - 1) * stride + col)])) { psis_rest_fold(-v, m_rest, r_rest); continue; }
      const double out = psis_insert(keep.data() + col, stride, (int)K1, v);
      if (out != INFINITY) psis_rest_fold(-out, m_rest, r_rest);
    }
    for (int64_t j = 0; j < K1; ++j)
      for (int64_t cc = 0; cc < stride; ++cc)
        if (cc != col && keep[(size_t)(j * stride + cc)] != SENTINEL) return 3;
    double work[PSIS_WORK];
    const PsisOut o = psis_finish(keep.data() + col, stride, (int)K1, m_rest, r_rest, S, work, 1);
    std::printf("%a %a %a %a\n", o.khat, o.elpd, m_rest, r_rest);
  }
  return 0;
}
