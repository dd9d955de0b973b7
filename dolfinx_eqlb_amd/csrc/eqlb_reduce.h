// The fixed-order block reduction of the streaming kernels (eqlb_marking.hip, eqlb_primal_solve.hip): NCH channels of
// THREADS per-thread partials in LDS, added by one tree whose pairs do not depend on the data or on scheduling - two
// calls on the same input give the same bits.  Device code only.
//
// A macro, not a function: as an inlined function template over a reference to the LDS array the same loop compiled
// to other code in k_indicator_total (722 -> 777 instructions) and k_indicator_reduce (863 -> 870); the text below is
// the loop those kernels always had, and tools/isa_compare.py shows their code unchanged.
#pragma once

// sh[j][0] = sum of sh[j][0 .. THREADS) for the channels j < NCH of the LDS array sh [..][THREADS]; every thread t of
// the block runs it after a barrier that made the partials visible, and may read sh[j][0] behind it
#define EQLB_BLOCK_TREE_SUM(sh, t, NCH, THREADS)                                                                       \
  for (int s = (THREADS) / 2; s >= 1; s >>= 1)                                                                         \
  {                                                                                                                    \
    if (t < s)                                                                                                         \
    {                                                                                                                  \
      _Pragma("unroll") for (int j = 0; j < (NCH); ++j) sh[j][t] += sh[j][t + s];                                      \
    }                                                                                                                  \
    __syncthreads();                                                                                                   \
  }
