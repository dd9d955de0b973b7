// The host-side planning of the CSR pattern build (eqlb_primal_matrix.hip): sizes, the bits of the sort and the guards
// of the index types.  Plain C++ with no device call, so that a stand-alone program can run it under a sanitizer
// (tools/matrix_plan_check.cpp, built and run by tests/test_primal_matrix_host.py).
#pragma once

#include <cstddef>
#include <cstdint>

namespace eqlb
{
struct MatrixPlan
{
  bool ok = false;       // rows fit the int32 column indices, the keys fit 64 bits
  int64_t rows = 0;      // bs * ndofs
  int64_t nkeys = 0;     // ncells * nd_p^2 pairs before the sort
  unsigned key_bits = 0; // bits of the largest key ndofs^2 - 1
};

inline unsigned matrix_bits_of(unsigned long long v) // bits needed for the values 0 ... v
{
  unsigned b = 1;
  while (b < 64 && (v >> b))
    ++b;
  return b;
}

inline MatrixPlan matrix_plan(int bs, int nd, int64_t ncells, int64_t ndofs)
{
  MatrixPlan p;
  if (bs < 1 || bs > 2 || nd < 1 || nd > 15 || ncells < 1 || ndofs < 1)
    return p;
  if (ndofs > INT32_MAX / bs || ncells > INT32_MAX)
  {
    p.rows = ndofs > INT64_MAX / bs ? INT64_MAX : bs * ndofs;
    p.nkeys = ncells > INT64_MAX / (nd * nd) ? INT64_MAX : ncells * nd * nd;
    return p;
  }
  p.rows = bs * ndofs;
  p.nkeys = ncells * nd * nd; // < 2^31 * 225
  p.key_bits = matrix_bits_of((unsigned long long)ndofs * (unsigned long long)ndofs - 1ull); // ndofs < 2^31
  p.ok = true;
  return p;
}

// bs * bs * snnz entries are counted in int64
inline bool matrix_count_fits(int bs, int64_t snnz) { return snnz >= 0 && snnz <= INT64_MAX / (bs * bs); }

// bytes of the arrays a pattern keeps: sptr [ndofs + 1] int64, srow and scol [snnz] int32
inline size_t matrix_kept_bytes(int64_t ndofs, int64_t snnz)
{
  return ((size_t)ndofs + 1) * sizeof(int64_t) + 2 * (size_t)snnz * sizeof(int32_t);
}
} // namespace eqlb
