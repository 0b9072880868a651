// A stand-alone host program around pymc_amd/csrc/predict.h (tests/test_predict_host.py builds it with the system compiler,
// warnings as errors, address and undefined-behaviour sanitizers where they link).  Standard input, one request after another:
//   mom dist a1 a2 a3                          -> mean var
//   mix K mu_0.. sigma_0.. w_0..               -> mean var of the Normal mixture
//   fold S with_lp  m_0 v_0 lp_0  m_1 ...      -> mean M2 vbar lmax lsum count lpd after folding the S triples in order
// Doubles as strtod reads them (hex floats, nan, inf); results as hex floats (or nan / inf / -inf).  Exit status 2: malformed
// input; 4: a refused family.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "predict.h"

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

static long need_int(long lo, long hi) {
  std::string tok;
  if (!next_token(tok)) std::exit(2);
  char* end = nullptr;
  const long v = std::strtol(tok.c_str(), &end, 0);
  if (end == tok.c_str() || *end != '\0' || v < lo || v > hi) std::exit(2);
  return v;
}

static void put(double v) {
  if (v != v) std::printf("nan ");
  else if (v == INFINITY) std::printf("inf ");
  else if (v == -INFINITY) std::printf("-inf ");
  else std::printf("%a ", v);
}

int main() {
  std::string what;
  while (next_token(what)) {
    if (what == "mom") {
      const int dist = (int)need_int(-1000, 1000);
      const double a1 = need_double(), a2 = need_double(), a3 = need_double();
      if (!pd_family_ok(dist)) return 4;
      double m, v;
      pd_moments(dist, 0.0, a1, a2, a3, &m, &v);
      put(m); put(v);
    } else if (what == "mix") {
      const int K = (int)need_int(1, 16);
      std::vector<double> p(3 * (size_t)K);
      for (double& x : p) x = need_double();
      double m, v;
      pd_mixture(K, p.data(), p.data() + K, p.data() + 2 * K, &m, &v);
      put(m); put(v);
    } else if (what == "fold") {
      const long S = need_int(0, 1000000);
      const bool with_lp = need_int(0, 1) != 0;
      PDAcc a = pd_acc_init();
      for (long s = 0; s < S; ++s) {
        const double m = need_double(), v = need_double(), lp = need_double();
        pd_fold(&a, m, v, lp, with_lp);
      }
      put(a.mean); put(a.M2); put(a.vbar); put(a.lmax); put(a.lsum); put(a.count); put(pd_lpd(&a));
    } else return 2;
    std::printf("\n");
  }
  return 0;
}
