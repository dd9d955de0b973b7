// The coefficient rules of dolfinx_eqlb_amd/csrc/eqlb_cell_coeff.h, printed by a program of its own: the header is all
// it includes of the library, so it builds with any host compiler and runs under the sanitizers
// (tests/test_cell_coeff_host.py holds the lines this prints).
#include "../dolfinx_eqlb_amd/csrc/eqlb_cell_coeff.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include <vector>

using namespace eqlb;

static const char* fault_name(TensorFault f)
{
  return f == TensorFault::none ? "ok" : f == TensorFault::not_finite ? "not finite" : "not definite";
}

// n good entries of the coefficient, then the listed ones made bad
static std::vector<double> entries(const CellCoeff& c, long long n, std::initializer_list<long long> bad)
{
  std::vector<double> a((size_t)(n * c.width()));
  for (long long i = 0; i < n; ++i)
    if (c.rule)
      a[i] = 1.0;
    else
      a[3 * i] = a[3 * i + 2] = 1.0; // (d01 = 0: the identity)
  for (long long i : bad)
    a[c.width() * i] = -1.0; // breaks each of the three scalar rules, and d00 > 0
  return a;
}

int main()
{
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double values[10] = {-inf, -1.0, std::nextafter(-1.0, 0.0), -0.0, 0.0, std::numeric_limits<double>::denorm_min(),
                             1.0,  DBL_MAX, inf, nan};
  const struct
  {
    const char* name;
    const ScalarRule* rule;
  } rules[3] = {{"non-negative", &NON_NEGATIVE}, {"positive", &POSITIVE}, {"above -1", &ABOVE_MINUS_ONE}};
  for (const auto& r : rules)
  {
    printf("rule %s:", r.name);
    for (double v : values)
      printf(" %d", r.rule->ok(v) ? 1 : 0);
    printf("\n");
  }

  const double tensors[8][3] = {{1.0, 0.0, 1.0}, {1.0, 1.0, 1.0}, {0.0, 0.0, 1.0},  {-1.0, 0.0, -1.0},
                                {1.0, nan, 1.0}, {inf, 0.0, 1.0}, {nan, 0.0, -1.0}, {1e-200, 0.0, 1e-200}};
  for (const auto& t : tensors)
    printf("tensor (%g, %g, %g): %s\n", t[0], t[1], t[2], fault_name(tensor_fault(t[0], t[1], t[2])));

  // the first bad cell: nothing to read, one bad entry, two bad entries, the last entry alone
  for (const CellCoeff* c : {&CELL_C, &CELL_MU, &CELL_PI1, &CELL_D})
  {
    const std::vector<double> one = entries(*c, 1, {0}), two = entries(*c, 10, {3, 7}), last = entries(*c, 10, {9}),
                              good = entries(*c, 10, {});
    printf("scan %s: %lld %lld %lld %lld %lld\n", c->name, c->first_bad(nullptr, 0), c->first_bad(one.data(), 1),
           c->first_bad(two.data(), 10), c->first_bad(last.data(), 10), c->first_bad(good.data(), 10));
  }

  // the messages, one of each form
  char msg[256];
  const double neg = -1.0, zero = 0.0;
  format_scalar(msg, sizeof(msg), "eqlb_x", "c", NON_NEGATIVE, neg);
  puts(msg);
  format_scalar(msg, sizeof(msg), "eqlb_x", "alpha", NON_NEGATIVE, inf);
  puts(msg);
  format_scalar(msg, sizeof(msg), "eqlb_x", "mu", POSITIVE, zero);
  puts(msg);
  std::vector<double> a(12, 1.0);
  a[3] = -0.5;
  format_cell(msg, sizeof(msg), "eqlb_x", CELL_C, a.data(), 3);
  puts(msg);
  a[0] = -2.0;
  format_cell(msg, sizeof(msg), "eqlb_x", FACET_ALPHA, a.data(), 0);
  puts(msg);
  a[11] = -1.0;
  format_cell(msg, sizeof(msg), "eqlb_x", CELL_MU, a.data(), 11);
  puts(msg);
  a[2] = 0.0;
  format_cell(msg, sizeof(msg), "eqlb_x", CELL_COEFF, a.data(), 2);
  puts(msg);
  a[4] = -1.0;
  format_cell(msg, sizeof(msg), "eqlb_x", CELL_PI1, a.data(), 4);
  puts(msg);
  const double D[9] = {1.0, 0.0, 1.0, 1.0, inf, 1.0, 1.0, 2.0, 1.0};
  format_cell(msg, sizeof(msg), "eqlb_x", CELL_D, D, 1);
  puts(msg);
  format_cell(msg, sizeof(msg), "eqlb_x", CELL_D, D, 2);
  puts(msg);
  return 0;
}
