// A stand-alone host program around psis_fit / psis_weight of pymc_amd/csrc/psis.h (tests/test_loo_pit_host.py builds it with the
// system compiler, warnings as errors, address and undefined-behaviour sanitizers where they link).  Standard input, one case
// after another:
//   S reff stride column v_0 ... v_{S-1} Q u_0 ... u_{Q-1}      (values as strtod reads them: hex floats, nan, inf, -inf)
// The S values are folded draw by draw into column `column` of a [K1][stride] block exactly as k_psis_fold folds them and fitted;
// then every one of them, in draw order, and the Q further values are weighted one by one, as k_loo_weight does.  Standard output
// per case, as hex floats: state khat elpd_loo_i (psis_finish's) c xc tl sigma logden, then the S + Q weights.  Exit status 2:
// malformed input; 3: a neighbouring column of the block was written; 4: psis_fit and psis_finish disagree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); }

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
    std::vector<double> keep((size_t)(K1 * stride), SENTINEL), v((size_t)S);
    for (int64_t j = 0; j < K1; ++j) keep[(size_t)(j * stride + col)] = INFINITY;
    double m_rest = -INFINITY, r_rest = 0.0;
    for (int64_t s = 0; s < S; ++s) {
      if (!next_double(v[(size_t)s])) return 2;
      const double x = v[(size_t)s];
      if (!(x < keep[(size_t)((K1 - 1) * stride + col)])) { psis_rest_fold(-x, m_rest, r_rest); continue; }
      const double out = psis_insert(keep.data() + col, stride, (int)K1, x);
      if (out != INFINITY) psis_rest_fold(-out, m_rest, r_rest);
    }
    double q_in;
    if (!next_double(q_in) || q_in < 0.0) return 2;
    const int64_t Q = (int64_t)q_in;
    std::vector<double> u((size_t)Q);
    for (int64_t k = 0; k < Q; ++k)
      if (!next_double(u[(size_t)k])) return 2;
    for (int64_t j = 0; j < K1; ++j)
      for (int64_t cc = 0; cc < stride; ++cc)
        if (cc != col && keep[(size_t)(j * stride + cc)] != SENTINEL) return 3;
    double work[PSIS_WORK];
    const PsisFit f = psis_fit(keep.data() + col, stride, (int)K1, m_rest, r_rest, S, work, 1);
    const PsisOut o = psis_finish(keep.data() + col, stride, (int)K1, m_rest, r_rest, S, work, 1);
    if (f.state == PSIS_FIT_OK ? !same_bits(f.khat, o.khat) : (f.state == PSIS_FIT_DEGENERATE ? o.elpd != -INFINITY : o.elpd == o.elpd)) return 4;
    std::printf("%a %a %a %a %a %a %a %a", (double)f.state, o.khat, o.elpd, f.c, f.xc, (double)f.tl, f.sigma, f.logden);
    for (int64_t s = 0; s < S; ++s) std::printf(" %a", psis_weight(f, keep.data() + col, stride, v[(size_t)s]));
    for (int64_t k = 0; k < Q; ++k) std::printf(" %a", psis_weight(f, keep.data() + col, stride, u[(size_t)k]));
    std::printf("\n");
  }
  return 0;
}
