// The plan behind eqlb_refine_t: what eqlb_mesh_refine_plan keeps on the device (eqlb_mesh_refine.hip) and what the
// transfer entries read from it (eqlb_transfer.hip).  Host code only.
#pragma once

#include "eqlb_mesh_handle.h" // (eqlb_host_util.h)

struct eqlb_refine
{
  const eqlb_mesh* mesh = nullptr;
  int32_t nnodes = 0, ncells = 0, nfacets = 0;
  int32_t nbis = 0, ncells2 = 0, ncut = 0;
  eqlb::DevBuf<int32_t> fE, frank; // [nfacets + 1] flag of E; exclusive scan: rank among E
  eqlb::DevBuf<int32_t> bis_facet; // [nbis] of [nfacets]: the facets of E, ascending
  eqlb::DevBuf<uint32_t> coff;     // [ncells + 1] first child
  eqlb::DevBuf<uint8_t> lloc;      // [ncells] l(c)
};
