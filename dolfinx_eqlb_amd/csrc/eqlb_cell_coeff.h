// The admission rules of the cell-wise (and facet-wise) coefficients of the P_p chain, ONCE: what a host array or a
// scalar must satisfy before a handle or anything on the device changes, which entry breaks the rule first, and the
// message that says so.  include/eqlb.h states the rules per entry point; the numpy validators of cpp.py and
// lsolver/primal.py are the statement the device path is compared against.
//
// Pure host C++17 without a HIP header: eqlb_host_util.h wraps it for the units of the library (check_scalar,
// check_cells, fail_cell), tools/cell_coeff_check.cpp includes it alone (tests/test_cell_coeff_host.py).  A new
// coefficient adds its CellCoeff line here - and a ScalarRule only if none of the three fits.  Everything lies in an
// unnamed namespace, as the host helpers of the units do: the library exports none of it.
#pragma once

#include <cmath>
#include <cstdio>

namespace eqlb
{
namespace
{
// a rule for one number: the predicate and the sentence that ends the message of a number that fails it
struct ScalarRule
{
  bool (*ok)(double);
  const char* sentence;
};
inline bool rule_non_negative(double x) { return x >= 0.0 && std::isfinite(x); }
inline bool rule_positive(double x) { return x > 0.0 && std::isfinite(x); }
inline bool rule_above_minus_one(double x) { return x > -1.0; }
constexpr ScalarRule NON_NEGATIVE{rule_non_negative, "is negative, NaN or infinite"};
constexpr ScalarRule POSITIVE{rule_positive, "is zero, negative, NaN or infinite"};
constexpr ScalarRule ABOVE_MINUS_ONE{rule_above_minus_one, "is not above -1"};

// the rule for a symmetric tensor (d00, d01, d11): finite, then d00 > 0 and d00 d11 - d01^2 > 0 with the products
// rounded as written here.  The reason that comes first is the one reported
enum class TensorFault
{
  none,
  not_finite,
  not_definite
};
inline TensorFault tensor_fault(double d00, double d01, double d11)
{
  if (!(std::isfinite(d00) && std::isfinite(d01) && std::isfinite(d11)))
    return TensorFault::not_finite;
  if (!(d00 > 0.0 && d00 * d11 - d01 * d01 > 0.0))
    return TensorFault::not_definite;
  return TensorFault::none;
}
inline const char* tensor_sentence(TensorFault f)
{
  return f == TensorFault::not_finite ? "is not finite" : "is not positive definite";
}

// the first i of a[0 .. n) that breaks the rule, or -1; n <= 0 reads nothing
inline long long first_bad(const ScalarRule& rule, const double* a, long long n)
{
  for (long long i = 0; i < n; ++i)
    if (!rule.ok(a[i]))
      return i;
  return -1;
}
// the same for tensors D [n][3]
inline long long first_bad_tensor(const double* D, long long n)
{
  for (long long i = 0; i < n; ++i)
    if (tensor_fault(D[3 * i], D[3 * i + 1], D[3 * i + 2]) != TensorFault::none)
      return i;
  return -1;
}

// a coefficient array as the messages name it, with its rule; rule == nullptr: the tensor rule on [n][3]
struct CellCoeff
{
  const char* name;
  const ScalarRule* rule;
  int width() const { return rule ? 1 : 3; }
  long long first_bad(const double* a, long long n) const
  {
    return rule ? eqlb::first_bad(*rule, a, n) : first_bad_tensor(a, n);
  }
};
constexpr CellCoeff CELL_C{"cell_c", &NON_NEGATIVE};           // the reaction term
constexpr CellCoeff FACET_ALPHA{"facet_alpha", &NON_NEGATIVE}; // the Robin term, per listed facet
constexpr CellCoeff CELL_MU{"cell_mu", &POSITIVE};             // the shear modulus
constexpr CellCoeff CELL_COEFF{"cell_coeff", &POSITIVE};       // the weight of the estimators
constexpr CellCoeff CELL_PI1{"cell_pi1", &ABOVE_MINUS_ONE};    // pi_1 of the stress estimator
constexpr CellCoeff CELL_D{"cell_D", nullptr};                 // the diffusion tensor

// the messages: `who` is the entry point.  "<who>: <name> = <x> <sentence>" for a scalar ...
inline int format_scalar(char* buf, size_t cap, const char* who, const char* name, const ScalarRule& rule, double x)
{
  return snprintf(buf, cap, "%s: %s = %g %s", who, name, x, rule.sentence);
}
// ... and "<who>: <name>[<i>] = <entry> <sentence>" for entry i of an array that breaks its rule
inline int format_cell(char* buf, size_t cap, const char* who, const CellCoeff& c, const double* a, long long i)
{
  if (c.rule)
    return snprintf(buf, cap, "%s: %s[%lld] = %g %s", who, c.name, i, a[i], c.rule->sentence);
  const double* d = a + 3 * i;
  return snprintf(buf, cap, "%s: %s[%lld] = (%g, %g, %g) %s", who, c.name, i, d[0], d[1], d[2],
                  tensor_sentence(tensor_fault(d[0], d[1], d[2])));
}
} // namespace
} // namespace eqlb
