// Stand-alone check of the host-side planning of the CSR pattern build (dolfinx_eqlb_amd/csrc/eqlb_matrix_plan.h):
// sizes, the bits of the sort and the guards of the index types, at the edges of the ranges.  Built by
// tests/test_primal_matrix_host.py with -fsanitize=address,undefined where the compiler has the runtimes.  Prints one
// line per case: bs nd ncells ndofs -> ok rows nkeys key_bits, then the cases of the count guard.
#include "../dolfinx_eqlb_amd/csrc/eqlb_matrix_plan.h"

#include <cstdio>
#include <vector>

int main()
{
  using namespace eqlb;
  struct Case
  {
    int bs, nd;
    int64_t ncells, ndofs;
  };
  const std::vector<Case> cases = {
      {1, 3, 1, 3},                            // one cell
      {1, 15, 1000000, 8004001},               // P_4 at 1M cells: 225M keys
      {2, 15, 1000000, 8004001},
      {1, 3, INT32_MAX, INT32_MAX},            // the last count that fits: keys of 62 bits
      {2, 3, 100, (int64_t)INT32_MAX / 2},     // 2 ndofs = 2^31 - 2 fits
      {2, 3, 100, (int64_t)INT32_MAX / 2 + 1}, // 2 ndofs = 2^31 does not
      {1, 3, 100, (int64_t)INT32_MAX + 1},
      {1, 3, (int64_t)INT32_MAX + 1, 100},
      {1, 15, INT64_MAX, INT64_MAX},           // nothing overflows on the way to the refusal
      {2, 15, INT64_MAX, INT64_MAX},
      {0, 3, 1, 3},
      {3, 3, 1, 3},
      {1, 0, 1, 3},
      {1, 16, 1, 3},
      {1, 3, 0, 3},
      {1, 3, 1, 0},
      {1, 3, -1, -1},
  };
  for (const Case& c : cases)
  {
    const MatrixPlan p = matrix_plan(c.bs, c.nd, c.ncells, c.ndofs);
    std::printf("%d %d %lld %lld -> %d %lld %lld %u\n", c.bs, c.nd, (long long)c.ncells, (long long)c.ndofs, p.ok ? 1 : 0,
                (long long)p.rows, (long long)p.nkeys, p.key_bits);
  }
  const unsigned long long probes[] = {0ull, 1ull, 2ull, 3ull, 255ull, 256ull, (1ull << 62) - 1ull, 1ull << 62, ~0ull};
  for (unsigned long long v : probes)
    std::printf("bits %llu -> %u\n", v, matrix_bits_of(v));
  std::printf("count %d %d %d %d %d\n", matrix_count_fits(1, 0) ? 1 : 0, matrix_count_fits(2, INT64_MAX / 4) ? 1 : 0,
              matrix_count_fits(2, INT64_MAX / 4 + 1) ? 1 : 0, matrix_count_fits(1, INT64_MAX) ? 1 : 0,
              matrix_count_fits(1, -1) ? 1 : 0);
  std::printf("kept %zu\n", matrix_kept_bytes(8004001, 225000000));
  return 0;
}
