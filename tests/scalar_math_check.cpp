// Stand-alone host program around pymc_amd/csrc/scalar_math.h (tests/test_scalar_edges.py).
// stdin: one request per line, `function hexdouble [hexdouble]` (C99 hexadecimal floats, "nan", "inf"); stdout: the result of
// the header's function as a hexadecimal float, one line per request.  An unknown function or a malformed line ends the program
// with status 2.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scalar_math.h"

int main() {
  char line[256], name[32], sx[64], sy[64];
  while (fgets(line, sizeof line, stdin)) {
    const int n = sscanf(line, "%31s %63s %63s", name, sx, sy);
    if (n < 2) return 2;
    char* end = nullptr;
    const double x = strtod(sx, &end);
    if (*end) return 2;
    double y = 0.0;
    if (n == 3) {
      y = strtod(sy, &end);
      if (*end) return 2;
    }
    double r;
    if (!strcmp(name, "softplus") && n == 2) r = softplus_d(x);
    else if (!strcmp(name, "sigmoid") && n == 2) r = sigmoid_d(x);
    else if (!strcmp(name, "log1mexp") && n == 2) r = log1mexp_d(x);
    else if (!strcmp(name, "digamma") && n == 2) r = digamma_d(x);
    else if (!strcmp(name, "trigamma") && n == 2) r = trigamma_d(x);
    else if (!strcmp(name, "logaddexp") && n == 3) r = logaddexp_d(x, y);
    else return 2;
    printf("%a\n", r);
  }
  return 0;
}
