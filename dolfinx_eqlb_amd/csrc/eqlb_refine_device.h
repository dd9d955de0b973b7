// Device functions that the kernels behind eqlb_refine_* share (eqlb_mesh_refine.hip, eqlb_bc_carry.hip).
#pragma once

#include "eqlb_internal.h"

namespace eqlb
{
// The parent of facet f2 of the refined handle (eqlb_refine_parent_facets): the old facet with the same two nodes; the
// bisected old facet if one end is the new node of a facet that the other end belongs to; -1 otherwise.  The node
// indices of the refined handle are < nnodes + nbis (checked by the caller).
__device__ __forceinline__ int32_t parent_facet_of(int32_t f2, int32_t nnodes, const int32_t* __restrict__ facet_nodes2,
                                                   const int32_t* __restrict__ bis_facet,
                                                   const int32_t* __restrict__ facet_nodes,
                                                   const int32_t* __restrict__ node_facets_off,
                                                   const int32_t* __restrict__ node_facets)
{
  const int32_t n0 = facet_nodes2[2 * (int64_t)f2], n1 = facet_nodes2[2 * (int64_t)f2 + 1];
  const int32_t lo = n0 < n1 ? n0 : n1, hi = n0 < n1 ? n1 : n0;
  int32_t found = -1;
  if (hi < nnodes)
  {
    for (int32_t q = node_facets_off[lo]; q < node_facets_off[lo + 1] && found < 0; ++q)
    {
      const int32_t g = node_facets[q];
      const int32_t a = facet_nodes[2 * (int64_t)g], b = facet_nodes[2 * (int64_t)g + 1];
      if ((a == lo && b == hi) || (a == hi && b == lo))
        found = g;
    }
  }
  else if (lo < nnodes)
  {
    const int32_t g = bis_facet[hi - nnodes];
    if (facet_nodes[2 * (int64_t)g] == lo || facet_nodes[2 * (int64_t)g + 1] == lo)
      found = g;
  }
  return found;
}
} // namespace eqlb
