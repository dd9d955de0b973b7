// What the patch builder can walk.  eqlb_boundary_plan.h includes this file for the checks of eqlb_se_set_boundary
// (and through it eqlb_handle.h: eqlb_api.hip counts the one-cell facets of a mesh with it), and the stand-alone host
// programs tools/topology_check_emul.cpp and tools/boundary_plan_emul.cpp include it with a plain C++ compiler: it
// calls nothing of HIP.  The two per-node functions (count of one-cell facets, the walkable predicate) are also what
// the export launch of k_build_patches runs, so that host and kernel cannot drift apart; for that one use, and only when hipcc reads
// the file, the macro below marks them __host__ __device__.
//
// k_build_patches (eqlb_patch_builder.hip) walks the cells round a node from a start facet, crossing one facet per
// step.  That is defined for a closed ring of cells and for ONE open fan between two boundary facets, and for nothing
// else.  With n cells, nf facets and b one-cell facets at the node, every open fan at the node adds one facet more than
// cells and two one-cell facets, every closed ring as many facets as cells and no one-cell facet:
//
//        nf = n + (number of open fans),   b = 2 (number of open fans).
//
// In a planar conforming triangulation a closed ring surrounds its node, so it is the only component there; hence
// "walkable" = (nf == n and b == 0) or (nf == n + 1 and b == 2) is exactly "one closed ring or one open fan".  A node at
// which two fans meet (nf == n + 2, b == 4: a pinched, "bow-tie" vertex) is not walkable.  The walk of a boundary node
// starts at a typed one-cell facet and ends at the other one, so every one-cell facet of an equilibrated node must carry
// a type, and no two-cell facet may (it could be taken for the start facet).
#pragma once

#include <cstddef>
#include <cstdint>

// the per-node functions are shared with the kernel; a host compiler sees plain inline functions
#ifdef __HIPCC__
#define EQLB_TOPO_HD __host__ __device__
#else
#define EQLB_TOPO_HD
#endif

namespace eqlb
{

// number of one-cell facets among the nf facets of a node; facet_cells_off: CSR offsets of the facet -> cell table
EQLB_TOPO_HD inline int32_t node_boundary_facets(const int32_t* node_fcts, int32_t nf, const int32_t* facet_cells_off)
{
  int32_t b = 0;
  for (int32_t i = 0; i < nf; ++i)
    b += (facet_cells_off[node_fcts[i] + 1] - facet_cells_off[node_fcts[i]] == 1);
  return b;
}

// b [nnodes]: that count for every node
inline void count_node_boundary_facets(int32_t nnodes, const int32_t* node_facets_off, const int32_t* node_facets,
                                       const int32_t* facet_cells_off, int32_t* b)
{
  for (int32_t i = 0; i < nnodes; ++i)
    b[i] = node_boundary_facets(node_facets + node_facets_off[i], node_facets_off[i + 1] - node_facets_off[i],
                                facet_cells_off);
}

// one closed ring (n cells, n facets, none of them on the boundary) or one open fan (n cells, n + 1 facets, two of them
// on the boundary)
EQLB_TOPO_HD inline bool node_walkable(int32_t n, int32_t nf, int32_t b)
{
  return (nf == n && b == 0) || (nf == n + 1 && b == 2);
}

enum TopoVerdict : int
{
  TOPO_OK = 0,
  TOPO_NODE_NOT_WALKABLE = 1,       // index: the node
  TOPO_BOUNDARY_FACET_UNTYPED = 2,  // index: the facet, row: the right-hand side
  TOPO_INTERIOR_FACET_TYPED = 3     // index: the facet, row: the right-hand side
};

struct TopoFinding
{
  int verdict;
  int32_t index; // node or facet, -1 with TOPO_OK
  int32_t row;   // right-hand side of a facet finding, else 0
};

// The first offender, in this order: nodes in ascending order, then row by row the facets in ascending order.
// node_mask: nullptr = every node is equilibrated.  Nodes that are masked out are not looked at, nor are facets both
// of whose nodes are masked out (the rim of a rank's local mesh holds pinched nodes and artificial boundary facets).
// facet_type [nrhs][nfacets]: 0 = not on the boundary, 1 / 2 = the two kinds of boundary facets.
inline TopoFinding check_boundary_topology(int32_t nnodes, int32_t nfacets, int32_t nrhs, const int32_t* node_ncells,
                                           const int32_t* node_nfcts, const int32_t* node_nbnd,
                                           const int32_t* facet_nodes, const int32_t* facet_cells_off,
                                           const int8_t* facet_type, const uint8_t* node_mask)
{
  for (int32_t i = 0; i < nnodes; ++i)
    if ((!node_mask || node_mask[i]) && !node_walkable(node_ncells[i], node_nfcts[i], node_nbnd[i]))
      return {TOPO_NODE_NOT_WALKABLE, i, 0};
  for (int32_t r = 0; r < nrhs; ++r)
  {
    const int8_t* ft = facet_type + (size_t)r * nfacets;
    for (int32_t f = 0; f < nfacets; ++f)
    {
      const bool one_cell = facet_cells_off[f + 1] - facet_cells_off[f] == 1;
      if (one_cell == (ft[f] != 0))
        continue;
      if (node_mask && !node_mask[facet_nodes[2 * (size_t)f]] && !node_mask[facet_nodes[2 * (size_t)f + 1]])
        continue;
      return {one_cell ? TOPO_BOUNDARY_FACET_UNTYPED : TOPO_INTERIOR_FACET_TYPED, f, r};
    }
  }
  return {TOPO_OK, -1, 0};
}

} // namespace eqlb
