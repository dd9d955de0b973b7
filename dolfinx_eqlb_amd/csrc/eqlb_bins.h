// The lanes-per-patch bins and the limits that host planner, handles and kernels share.  Plain C++: included by
// eqlb_internal.h (every translation unit) and by eqlb_boundary_plan.h (also compiled by a host compiler alone).
#pragma once

#include <cstdint>

namespace eqlb
{

constexpr int MAX_BINS = 5;          // lanes per patch P = 4, 8, 16, 32, 64
constexpr int BIN_P[MAX_BINS] = {4, 8, 16, 32, 64};
constexpr int LARGE_MIN_CELLS = 64;  // a patch of that many cells (or of more than 64 facets) fits no bin
constexpr int WS_MAX_LEVELS = 4;     // levels of overlapping groups of boundary patches (stress path)

struct Bin
{
  int P = 0;
  int64_t npatch = 0;
  int64_t slot_offset = 0;   // into slot arrays
  int64_t patch_offset = 0;  // into patch arrays
  int64_t nfull = 0;         // fused stress tiles: the leading patches of the bin are the FULL ones (interior, as many
                             // cells as lanes) that the fused kernel takes; the slot path takes [nfull, npatch)
};

} // namespace eqlb
