// A stand-alone host program around pymc_amd/csrc/compare.h (tests/test_compare_host.py builds it with the system compiler, warnings as
// errors, address and undefined-behaviour sanitizers where they link).  Standard input, one request after another (numbers as strtod
// reads them):
//   G seed b0 nb i0 ni                 -> g(b, i) for b0 <= b < b0 + nb, i0 <= i < i0 + ni, replicate-major, as hex floats
//   T N K e[N][K]                      -> per observation m_i p_i0 .. p_i,K-1
//   P N K w[K] e[N][K]                 -> sum_i m_i, sum_i log d_i, g[K], H[K][K] at w
//   S N K tol max_passes e[N][K]       -> w[K], f(w), kkt_gap, passes
// Exit status 2: malformed input.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "compare.h"

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
  if (!next_token(tok)) std::exit(2);
  char* end = nullptr;
  const unsigned long long v = std::strtoull(tok.c_str(), &end, 0);
  if (end == tok.c_str() || *end != '\0') std::exit(2);
  return (uint64_t)v;
}

struct Problem {
  int64_t N;
  int K;
  std::vector<double> e, p;   // [N][K]
  double sum_m;
};

template <int K>
static void fill_terms(Problem& pr) {
  pr.sum_m = 0.0;
  for (int64_t i = 0; i < pr.N; ++i) {
    double x[K], t[K];
    for (int k = 0; k < K; ++k) x[k] = pr.e[(size_t)(i * K + k)];
    pr.sum_m += cmp_terms<K>(x, t);
    for (int k = 0; k < K; ++k) pr.p[(size_t)(i * K + k)] = t[k];
  }
}

template <int K>
static bool host_pass(void* ctx, const double* w, double* sums) {
  const Problem& pr = *static_cast<const Problem*>(ctx);
  double a[CMP_NACC(K)], wv[K];
  for (int j = 0; j < CMP_NACC(K); ++j) a[j] = 0.0;
  for (int k = 0; k < K; ++k) wv[k] = w[k];
  for (int64_t i = 0; i < pr.N; ++i) {
    double x[K];
    for (int k = 0; k < K; ++k) x[k] = pr.p[(size_t)(i * K + k)];
    cmp_pass_add<K>(x, wv, a);
  }
  for (int j = 0; j < CMP_NACC(K); ++j) sums[j] = a[j];
  return true;
}

#define DISPATCH(K, ...)                                                                                   \
  switch (K) {                                                                                             \
    case 2: { constexpr int KK = 2; __VA_ARGS__; } break; case 3: { constexpr int KK = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int KK = 4; __VA_ARGS__; } break; case 5: { constexpr int KK = 5; __VA_ARGS__; } break; \
    case 6: { constexpr int KK = 6; __VA_ARGS__; } break; case 7: { constexpr int KK = 7; __VA_ARGS__; } break; \
    default: { constexpr int KK = 8; __VA_ARGS__; } break;                                                 \
  }

static void read_problem(Problem& pr, bool with_w, double* w, double* tol, int* max_passes) {
  pr.N = (int64_t)need_double();
  pr.K = (int)need_double();
  if (pr.N < 1 || pr.N > 10000000 || pr.K < 2 || pr.K > CMP_MAXK) std::exit(2);
  if (with_w)
    for (int k = 0; k < pr.K; ++k) w[k] = need_double();
  if (tol) { *tol = need_double(); *max_passes = (int)need_double(); }
  pr.e.resize((size_t)(pr.N * pr.K));
  pr.p.resize(pr.e.size());
  for (double& v : pr.e) v = need_double();
  DISPATCH(pr.K, fill_terms<KK>(pr));
}

int main() {
  std::string cmd;
  while (next_token(cmd)) {
    if (cmd == "G") {
      const uint64_t seed = need_u64(), b0 = need_u64(), nb = need_u64(), i0 = need_u64(), ni = need_u64();
      for (uint64_t b = b0; b < b0 + nb; ++b) {
        for (uint64_t i = i0; i < i0 + ni; ++i) std::printf("%a ", cmp_g(seed, (int64_t)b, (int64_t)i));
        std::printf("\n");
      }
    } else if (cmd == "T") {
      Problem pr;
      read_problem(pr, false, nullptr, nullptr, nullptr);
      for (int64_t i = 0; i < pr.N; ++i) {
        double m = pr.e[(size_t)(i * pr.K)];
        for (int k = 1; k < pr.K; ++k) m = pr.e[(size_t)(i * pr.K + k)] > m ? pr.e[(size_t)(i * pr.K + k)] : m;
        std::printf("%a", m);
        for (int k = 0; k < pr.K; ++k) std::printf(" %a", pr.p[(size_t)(i * pr.K + k)]);
        std::printf("\n");
      }
    } else if (cmd == "P") {
      Problem pr;
      double w[CMP_MAXK], sums[CMP_NACC(CMP_MAXK)];
      read_problem(pr, true, w, nullptr, nullptr);
      DISPATCH(pr.K, host_pass<KK>(&pr, w, sums));
      CmpEval ev;
      cmp_unpack(pr.K, pr.N, sums, ev);
      std::printf("%a %a", pr.sum_m, ev.ld);
      for (int k = 0; k < pr.K; ++k) std::printf(" %a", ev.g[k]);
      for (int k = 0; k < pr.K; ++k)
        for (int l = 0; l < pr.K; ++l) std::printf(" %a", ev.H[k][l]);
      std::printf("\n");
    } else if (cmd == "S") {
      Problem pr;
      double tol = 0.0, w[CMP_MAXK], ld = 0.0, gap = 0.0;
      int max_passes = 0, passes = 0;
      read_problem(pr, false, nullptr, &tol, &max_passes);
      if (max_passes < 1) return 2;
      bool ok = false;
      DISPATCH(pr.K, ok = cmp_solve(KK, pr.N, host_pass<KK>, &pr, tol, max_passes, w, &ld, &gap, &passes));
      if (!ok) return 3;
      for (int k = 0; k < pr.K; ++k) std::printf("%a ", w[k]);
      std::printf("%a %a %d\n", pr.sum_m + ld, gap, passes);
    } else {
      return 2;
    }
  }
  return 0;
}
