// Transfer across one refinement level ON THE DEVICE: the P_p dofmap of a handle (eqlb_mesh_lagrange_dofmap) and the
// prolongation of P_p solutions and DG_d data from the mesh of a plan to its refined mesh (eqlb_refine_prolong_lagrange,
// eqlb_refine_prolong_dg) - what a DOLFINx caller gets from interpolating a Function of the old mesh into the space on
// the mesh of mesh.refine.  The rule is stated in include/eqlb.h and, as numpy, in dolfinx_eqlb_amd/mesh/transfer.py;
// the device reproduces the numpy statement bit for bit.
//
// The arithmetic is one table per degree q (tools/gen_tables.py: Prolong<q>, exact rationals): the values of the P_q
// basis functions at the half-spacing lattice of the reference triangle.  A child of one bisection level has vertices
// that are vertices or edge midpoints of its parent, so every DOF point of the child is a lattice point of the parent
// and its value is one row of the table applied to the parent's values.
//
// k_prolong<Q, DG>: ONE launch, one thread per PARENT cell, which walks its 1 ... 4 children (coff of the plan):
//  - the parent of a child is known without a search and the children's output rows are one contiguous piece; a thread
//    per child would have to look its parent up in coff (log2(ncells) dependent loads) - the plan keeps no parent table;
//  - the position of every child vertex in the parent comes from matching node ids (an old node: the parent's vertex
//    with that id; a new node: the midpoint of the ends of the facet it bisects, bis_facet of the plan) - integer work,
//    no coordinates; the lattice row of a local DOF is then q h_0 + a (h_1 - h_0) + b (h_2 - h_0);
//  - the rows differ from lane to lane, so the table cannot be read through scalar loads: it is staged in LDS once per
//    workgroup (45 x 15 doubles, 5.4 KB, at q = 4).  Lanes of copied cells read the same unit row (a broadcast);
//  - products are rounded one by one and added in ascending order (contraction switched off, as in k_facet_len2);
//  - P_p: only the OWNER of a global DOF stores it - the first cell of the node / facet in the refined handle's
//    node -> cell / facet -> cell table, the cell itself for interior DOFs - with plain stores.  No atomics, no
//    reduction across threads: the result does not depend on scheduling;
//  - every dofmap index is checked before it addresses anything: a parent with a bad index makes the DOFs its children
//    own NaN, a child with a bad index writes NaN to the in-range DOFs it owns and nothing else.
#include "eqlb_device_common.h"
#include "eqlb_refine_plan.h"
#include "eqlb_tables_gen.h"

#include <climits>

namespace eqlb
{
namespace
{
constexpr int TR_THREADS = 256;
constexpr int TR_PMAX = 4, TR_DMAX = 3;

// local DOF n of the equispaced P_Q (Basix order, elmtlib/lagrange.py) sits at (a[n], b[n]) / Q
template <int Q>
struct DofNum
{
  int a[nd_of(Q)], b[nd_of(Q)];
  constexpr DofNum() : a{}, b{}
  {
    int n = 0;
    a[n] = 0, b[n++] = 0;
    a[n] = Q, b[n++] = 0;
    a[n] = 0, b[n++] = Q;
    for (int i = 1; i < Q; ++i) // facet 0: vertex 1 -> vertex 2
      a[n] = Q - i, b[n++] = i;
    for (int i = 1; i < Q; ++i) // facet 1: vertex 0 -> vertex 2
      a[n] = 0, b[n++] = i;
    for (int i = 1; i < Q; ++i) // facet 2: vertex 0 -> vertex 1
      a[n] = i, b[n++] = 0;
    for (int j = 1; j < Q - 1; ++j)
      for (int i = 1; i < Q - j; ++i)
        a[n] = i, b[n++] = j;
  }
};

struct ProlongArgs
{
  int32_t ncells, nnodes, nbis, ncells2, nrhs, bs;
  // the old mesh and the plan
  const int32_t *cell_nodes, *facet_nodes, *bis_facet;
  const uint32_t* coff;
  // the refined handle
  const int32_t *cell_nodes2, *cell_facets2, *facet_cells_off2, *facet_cells2, *node_cells_off2, *node_cells2;
  // P_p: the caller's dofmaps
  const int32_t *cell_dofs, *cell_dofs2;
  int64_t ndofs, ndofs2;
  const double* in;
  double* out;
};

// h [3][2]: positions of the vertices w of a child in its parent with the vertices v, in half units; false if a
// vertex is neither a vertex nor an edge midpoint of the parent (a handle that is not the plan's refined mesh)
__device__ __forceinline__ bool child_positions(const ProlongArgs& a, const int32_t (&v)[3], const int32_t (&w)[3],
                                                int (&hx)[3], int (&hy)[3])
{
  bool found = true;
#pragma unroll
  for (int j = 0; j < 3; ++j)
  {
    const int32_t n = w[j];
    int32_t e0 = n, e1 = n;
    if (n >= a.nnodes)
    {
      e0 = e1 = -1;
      if (n - a.nnodes < a.nbis)
      {
        const int64_t f = a.bis_facet[n - a.nnodes];
        e0 = a.facet_nodes[2 * f];
        e1 = a.facet_nodes[2 * f + 1];
      }
    }
    int sx = 0, sy = 0, cnt = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) // parent vertices at (0,0), (2,0), (0,2)
    {
      const int k = (v[m] == e0) + (v[m] == e1);
      cnt += k;
      sx += (m == 1) ? 2 * k : 0;
      sy += (m == 2) ? 2 * k : 0;
    }
    found = found && cnt == 2;
    hx[j] = sx / 2;
    hy[j] = sy / 2;
  }
  return found;
}

template <int Q, bool DG>
__global__ void __launch_bounds__(TR_THREADS) k_prolong(const ProlongArgs a)
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  using T = eqlb_tables::Prolong<Q>;
  constexpr int ND = nd_of(Q), NROW = T::NROW;
  constexpr DofNum<Q> num{};
  static_assert(T::ND == ND && NROW == (2 * Q + 1) * (Q + 1), "table shape");
  __shared__ double sT[NROW * ND];
  for (int i = threadIdx.x; i < NROW * ND; i += TR_THREADS)
    sT[i] = T::PT[i];
  __syncthreads();
  const int32_t c = blockIdx.x * TR_THREADS + threadIdx.x;
  if (c >= a.ncells)
    return;
  const int32_t v[3] = {a.cell_nodes[3 * (int64_t)c], a.cell_nodes[3 * (int64_t)c + 1], a.cell_nodes[3 * (int64_t)c + 2]};
  const int64_t first = a.coff[c];
  const int nchild = (int)(a.coff[c + 1] - a.coff[c]); // 1 ... 4
  const double bad = __longlong_as_double(0x7ff8000000000000ll);
  int32_t idx[ND];
  bool ok = true;
  if constexpr (!DG)
  {
#pragma unroll
    for (int i = 0; i < ND; ++i)
    {
      idx[i] = a.cell_dofs[(int64_t)c * ND + i];
      ok = ok && idx[i] >= 0 && (int64_t)idx[i] < a.ndofs;
    }
  }
  for (int k = 0; k < nchild; ++k)
  {
    const int64_t c2 = first + k;
    const int32_t w[3] = {a.cell_nodes2[3 * c2], a.cell_nodes2[3 * c2 + 1], a.cell_nodes2[3 * c2 + 2]};
    int hx[3], hy[3];
    const bool found = child_positions(a, v, w, hx, hy);
    // lattice row of local DOF n: a point of the parent, 0 <= row < NROW
    auto row_of = [&](int n) {
      const int lx = Q * hx[0] + num.a[n] * (hx[1] - hx[0]) + num.b[n] * (hx[2] - hx[0]);
      const int ly = Q * hy[0] + num.a[n] * (hy[1] - hy[0]) + num.b[n] * (hy[2] - hy[0]);
      return found ? ly * (2 * Q + 1) - ly * (ly - 1) / 2 + lx : 0;
    };
    if constexpr (DG)
    {
      for (int r = 0; r < a.nrhs; ++r)
        for (int b = 0; b < a.bs; ++b)
        {
          const double* src = a.in + (((int64_t)r * a.ncells + c) * ND) * a.bs + b;
          double* dst = a.out + (((int64_t)r * a.ncells2 + c2) * ND) * a.bs + b;
          double vp[ND];
#pragma unroll
          for (int i = 0; i < ND; ++i)
            vp[i] = src[(int64_t)i * a.bs];
#pragma unroll 1 // (unrolled, the ND * ND table reads are hoisted into registers: 256 VGPRs at degree 3)
          for (int n = 0; n < ND; ++n)
          {
            const double* t = sT + row_of(n) * ND;
            double s = t[0] * vp[0];
#pragma unroll
            for (int i = 1; i < ND; ++i)
              s = s + t[i] * vp[i];
            dst[(int64_t)n * a.bs] = found ? s : bad;
          }
        }
    }
    else
    {
      // the child's own row of the dofmap, and which of its DOFs it owns
      int32_t idx2[ND];
      bool ok2 = true;
#pragma unroll
      for (int n = 0; n < ND; ++n)
      {
        idx2[n] = a.cell_dofs2[c2 * ND + n];
        ok2 = ok2 && idx2[n] >= 0 && (int64_t)idx2[n] < a.ndofs2;
      }
      bool own_v[3], own_f[3] = {true, true, true};
#pragma unroll
      for (int j = 0; j < 3; ++j)
        own_v[j] = a.node_cells2[a.node_cells_off2[w[j]]] == c2;
      if constexpr (Q > 1)
      {
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
          const int32_t f = a.cell_facets2[3 * c2 + j];
          own_f[j] = a.facet_cells2[a.facet_cells_off2[f]] == c2;
        }
      }
      const bool good = ok && ok2 && found;
      for (int r = 0; r < a.nrhs; ++r)
        for (int b = 0; b < a.bs; ++b)
        {
          const double* src = a.in + (int64_t)r * a.ndofs * a.bs + b;
          double* dst = a.out + (int64_t)r * a.ndofs2 * a.bs + b;
          double vp[ND];
#pragma unroll
          for (int i = 0; i < ND; ++i)
            vp[i] = ok ? src[(int64_t)idx[i] * a.bs] : 0.0;
#pragma unroll
          for (int n = 0; n < ND; ++n)
          {
            const bool own = n < 3 ? own_v[n] : (n < 3 * Q ? own_f[(n - 3) / (Q > 1 ? Q - 1 : 1)] : true);
            if (!own || idx2[n] < 0 || (int64_t)idx2[n] >= a.ndofs2)
              continue;
            const double* t = sT + row_of(n) * ND;
            double s = t[0] * vp[0];
#pragma unroll
            for (int i = 1; i < ND; ++i)
              s = s + t[i] * vp[i];
            dst[(int64_t)idx2[n] * a.bs] = good ? s : bad;
          }
        }
    }
  }
}

// The store pass of r = P^T r2, the transpose of k_prolong<Q, false> (include/eqlb.h: eqlb_hierarchy_restrict; the numpy
// statement: mesh/transfer.py: restrict_lagrange): one thread per PARENT cell, which walks its 1 ... 4 children and,
// within a child, the local DOFs that child owns - the owner test of k_prolong, so every fine DOF is taken once - and
// adds PT[row][i] * r2[dof2] to its ND x BS sums in registers; the sums go to the row of y_loc [ncells][ND][BS] the
// cell owns, with plain stores.  The owner sum of the coarse solver handle adds the rows up: no atomics anywhere.
// The table is staged in LDS as in k_prolong (the rows differ from lane to lane); the loop over the local DOFs is not
// unrolled (the row, the index and the owner bit of DOF n are looked up, the ND sums stay in registers).  a.in = r2,
// a.out = y_loc, a.cell_dofs2 / a.ndofs2 the fine dofmap; a bad index or a child that is no child of its parent makes
// the row of the cell NaN.
// R columns (BS = 1 only): r2 [R][ndofs2] -> y_loc [R][ncells][ND].  The children, their owner bits, the indices and
// the table rows are found once per cell and applied to the columns; the sum of a column runs in the one order.  The
// columns that run are those of cols (eqlb_internal.h: inside a batch of CG iterations a column whose stop flag is set
// is left alone - nothing reads its result); the others are neither read nor written.
template <int Q, int BS, int R>
__global__ void __launch_bounds__(TR_THREADS) k_restrict(const ProlongArgs a, const ManyCols cols, int64_t ystride)
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  using T = eqlb_tables::Prolong<Q>;
  constexpr int ND = nd_of(Q), NROW = T::NROW;
  constexpr int NV = BS * R; // values per fine DOF: the components of the one column, or the columns
  static constexpr DofNum<Q> num{}; // (indexed by a run-time n: a table in constant memory, not a private copy)
  static_assert(T::ND == ND && NROW == (2 * Q + 1) * (Q + 1), "table shape");
  static_assert(BS == 1 || R == 1, "columns for scalar spaces only");
  __shared__ double sT[NROW * ND];
  const uint32_t live = cols_live<R>(cols);
  if (!live)
    return;
  for (int i = threadIdx.x; i < NROW * ND; i += TR_THREADS)
    sT[i] = T::PT[i];
  __syncthreads();
  const int32_t c = blockIdx.x * TR_THREADS + threadIdx.x;
  if (c >= a.ncells)
    return;
  const int32_t v[3] = {a.cell_nodes[3 * (int64_t)c], a.cell_nodes[3 * (int64_t)c + 1], a.cell_nodes[3 * (int64_t)c + 2]};
  const int64_t first = a.coff[c];
  const int nchild = (int)(a.coff[c + 1] - a.coff[c]); // 1 ... 4
  double acc[ND][NV];
#pragma unroll
  for (int i = 0; i < ND; ++i)
#pragma unroll
    for (int b = 0; b < NV; ++b)
      acc[i][b] = 0.0;
  bool started = false, good = true;
  for (int j = 0; j < nchild; ++j)
  {
    const int64_t c2 = first + j;
    const int32_t w[3] = {a.cell_nodes2[3 * c2], a.cell_nodes2[3 * c2 + 1], a.cell_nodes2[3 * c2 + 2]};
    int hx[3], hy[3];
    const bool found = child_positions(a, v, w, hx, hy);
    good = good && found;
    // bit n: the child owns its local DOF n (interior DOFs: always)
    uint32_t own = ~0u << (3 * Q);
#pragma unroll
    for (int e = 0; e < 3; ++e)
      own |= (a.node_cells2[a.node_cells_off2[w[e]]] == c2) ? (1u << e) : 0u;
    if constexpr (Q > 1)
    {
#pragma unroll
      for (int e = 0; e < 3; ++e)
      {
        const int32_t f = a.cell_facets2[3 * c2 + e];
        const uint32_t bits = ((1u << (Q - 1)) - 1u) << (3 + e * (Q - 1));
        own |= (a.facet_cells2[a.facet_cells_off2[f]] == c2) ? bits : 0u;
      }
    }
#pragma unroll 1
    for (int n = 0; n < ND; ++n)
    {
      if (!((own >> n) & 1u))
        continue;
      const int32_t d2 = a.cell_dofs2[c2 * ND + n];
      if (d2 < 0 || (int64_t)d2 >= a.ndofs2)
      {
        good = false;
        continue;
      }
      const int lx = Q * hx[0] + num.a[n] * (hx[1] - hx[0]) + num.b[n] * (hx[2] - hx[0]);
      const int ly = Q * hy[0] + num.a[n] * (hy[1] - hy[0]) + num.b[n] * (hy[2] - hy[0]);
      const double* t = sT + (found ? ly * (2 * Q + 1) - ly * (ly - 1) / 2 + lx : 0) * ND;
      double rv[NV];
#pragma unroll
      for (int b = 0; b < NV; ++b)
      {
        if constexpr (R == 1)
          rv[b] = a.in[(int64_t)d2 * BS + b];
        else
          rv[b] = col_on<R>(live, b) ? a.in[b * a.ndofs2 + d2] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < ND; ++i)
      {
        const double ti = t[i];
#pragma unroll
        for (int b = 0; b < NV; ++b)
        {
          const double term = ti * rv[b];
          acc[i][b] = started ? acc[i][b] + term : term;
        }
      }
      started = true;
    }
  }
  const double bad = __longlong_as_double(0x7ff8000000000000ll);
  if constexpr (R == 1)
  {
    double* o = a.out + (int64_t)c * ND * BS;
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
      for (int b = 0; b < BS; ++b)
        o[i * BS + b] = good ? acc[i][b] : bad;
  }
  else
  {
#pragma unroll
    for (int k = 0; k < R; ++k)
    {
      if (!col_on<R>(live, k))
        continue;
      double* o = a.out + k * ystride + (int64_t)c * ND;
#pragma unroll
      for (int i = 0; i < ND; ++i)
        o[i] = good ? acc[i][k] : bad;
    }
  }
}

// DG_0: every child takes the value of its parent
__global__ void __launch_bounds__(TR_THREADS) k_prolong_dg0(const ProlongArgs a)
{
  const int32_t c = blockIdx.x * TR_THREADS + threadIdx.x;
  if (c >= a.ncells)
    return;
  const int64_t first = a.coff[c];
  const int nchild = (int)(a.coff[c + 1] - a.coff[c]);
  for (int r = 0; r < a.nrhs; ++r)
    for (int b = 0; b < a.bs; ++b)
    {
      const double val = a.in[((int64_t)r * a.ncells + c) * a.bs + b];
      for (int k = 0; k < nchild; ++k)
        a.out[((int64_t)r * a.ncells2 + first + k) * a.bs + b] = val;
    }
}

// one thread per cell: the row of the P_p dofmap in the numbering of mesh/transfer.py: lagrange_dofmap
__global__ void __launch_bounds__(TR_THREADS)
k_lagrange_dofmap(int32_t ncells, int32_t nnodes, int32_t nfacets, int p, const int32_t* __restrict__ cell_nodes,
                  const int32_t* __restrict__ cell_facets, const uint8_t* __restrict__ facet_perm,
                  int32_t* __restrict__ cell_dofs)
{
  const int32_t c = blockIdx.x * TR_THREADS + threadIdx.x;
  if (c >= ncells)
    return;
  const int ne = p - 1, ni = (p - 1) * (p - 2) / 2, nd = nd_of(p);
  int32_t* o = cell_dofs + (int64_t)c * nd;
  for (int j = 0; j < 3; ++j)
    o[j] = cell_nodes[3 * (int64_t)c + j];
  int col = 3;
  for (int f = 0; f < 3; ++f)
  {
    const int64_t base = (int64_t)nnodes + (int64_t)cell_facets[3 * (int64_t)c + f] * ne;
    const bool rev = facet_perm[3 * (int64_t)c + f] == 1;
    for (int j = 0; j < ne; ++j)
      o[col++] = (int32_t)(base + (rev ? ne - 1 - j : j));
  }
  const int64_t ibase = (int64_t)nnodes + (int64_t)nfacets * ne + (int64_t)c * ni;
  for (int j = 0; j < ni; ++j)
    o[col++] = (int32_t)(ibase + j);
}

template <bool DG>
void launch_prolong(int q, const ProlongArgs& a, hipStream_t stream)
{
  const dim3 grid(grid_of(a.ncells, TR_THREADS)), block(TR_THREADS);
  switch (q)
  {
  case 1:
    hipLaunchKernelGGL((k_prolong<1, DG>), grid, block, 0, stream, a);
    break;
  case 2:
    hipLaunchKernelGGL((k_prolong<2, DG>), grid, block, 0, stream, a);
    break;
  case 3:
    hipLaunchKernelGGL((k_prolong<3, DG>), grid, block, 0, stream, a);
    break;
  default:
    if constexpr (!DG) // DG data ends at degree 3
      hipLaunchKernelGGL((k_prolong<4, DG>), grid, block, 0, stream, a);
  }
}

// the arguments both prolongations share, after the checks both make
int common_args(const char* who, eqlb_refine_t* plan, eqlb_mesh_t* refined, int32_t bs, int32_t nrhs, int32_t memspace,
                ProlongArgs& a)
{
  if (bs < 1 || nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: bs = %d, nrhs = %d (both at least 1)", who, (int)bs, (int)nrhs);
  EQLB_TRY(check_memspace(who, memspace));
  const DeviceMesh &m = plan->mesh->m, &r = refined->m;
  if (r.nnodes != plan->nnodes + plan->nbis || r.ncells != plan->ncells2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: the handle has %d nodes and %d cells, the refined mesh %d and %d", who,
                r.nnodes, r.ncells, plan->nnodes + plan->nbis, plan->ncells2);
  a = ProlongArgs{};
  a.ncells = plan->ncells;
  a.nnodes = plan->nnodes;
  a.nbis = plan->nbis;
  a.ncells2 = plan->ncells2;
  a.nrhs = nrhs;
  a.bs = bs;
  a.cell_nodes = m.cell_nodes;
  a.facet_nodes = m.facet_nodes;
  a.bis_facet = plan->bis_facet.get();
  a.coff = plan->coff.get();
  a.cell_nodes2 = r.cell_nodes;
  a.cell_facets2 = r.cell_facets;
  a.facet_cells_off2 = r.facet_cells_off;
  a.facet_cells2 = r.facet_cells;
  a.node_cells_off2 = r.node_cells_off;
  return EQLB_OK;
}

int check_dofmap(const char* who, const char* name, const int32_t* cd, size_t ncells, int nd, int64_t ndofs)
{
  for (size_t i = 0; i < ncells * nd; ++i)
    if (cd[i] < 0 || (int64_t)cd[i] >= ndofs)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: %s[%lld][%d] = %d outside [0, %lld)", who, name, (long long)(i / nd),
                  (int)(i % nd), (int)cd[i], (long long)ndofs);
  return EQLB_OK;
}
} // namespace

// the store pass of the restriction for the hierarchy unit (eqlb_multilevel.hip) on the columns of c: DEVICE pointers,
// one launch
int launch_restrict(const char* who, eqlb_refine* plan, eqlb_mesh* refined, int p, int bs, const ManyCols& c,
                    const int32_t* cell_dofs2, int64_t ndofs2, const double* r2, double* yloc, hipStream_t stream)
{
  const int R = c.R;
  if (p < 1 || p > TR_PMAX || (bs != 1 && bs != 2))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: p = %d outside 1 ... 4, or bs = %d not 1 or 2", who, p, bs);
  if (R < 1 || R > MANY_R || (bs == 2 && R != 1))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: %d columns outside 1 ... 4 (bs = 2: one)", who, R);
  ProlongArgs a;
  EQLB_TRY(common_args(who, plan, refined, bs, R, EQLB_MEM_DEVICE, a));
  if (mesh_node_cells(refined, &a.node_cells2))
    return EQLB_ERR_DEVICE;
  a.cell_dofs2 = cell_dofs2;
  a.ndofs2 = ndofs2;
  a.in = r2;
  a.out = yloc;
  const int64_t ystride = (int64_t)a.ncells * nd_of(p);
  const dim3 grid(grid_of(a.ncells, TR_THREADS)), block(TR_THREADS);
  // slot 0 of a degree: bs = 2 (one column); slots 1 ... 4: the column counts of bs = 1
#define EQLB_RESTRICT_CASE(QQ, BB, RR)                                                                                 \
  case 5 * QQ + (BB == 2 ? 0 : RR):                                                                                    \
    hipLaunchKernelGGL((k_restrict<QQ, BB, RR>), grid, block, 0, stream, a, c, ystride);                               \
    break;
#define EQLB_RESTRICT_Q(QQ)                                                                                            \
  EQLB_RESTRICT_CASE(QQ, 1, 1) EQLB_RESTRICT_CASE(QQ, 1, 2) EQLB_RESTRICT_CASE(QQ, 1, 3) EQLB_RESTRICT_CASE(QQ, 1, 4)  \
  EQLB_RESTRICT_CASE(QQ, 2, 1)
  switch (5 * p + (bs == 2 ? 0 : R))
  {
    EQLB_RESTRICT_Q(1)
    EQLB_RESTRICT_Q(2)
    EQLB_RESTRICT_Q(3)
    EQLB_RESTRICT_Q(4)
  }
#undef EQLB_RESTRICT_Q
#undef EQLB_RESTRICT_CASE
  HIP_TRY(hipGetLastError());
  return EQLB_OK;
}
} // namespace eqlb

extern "C" {

int eqlb_mesh_lagrange_dofmap(eqlb_mesh_t* mesh, int32_t p, int32_t* cell_dofs, int64_t* ndofs_out, int32_t memspace,
                              void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_mesh_lagrange_dofmap";
  if (!mesh || !cell_dofs)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (p < 1 || p > TR_PMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: p = %d outside 1 ... 4", who, (int)p);
  EQLB_TRY(check_memspace(who, memspace));
  const DeviceMesh& m = mesh->m;
  const int ne = p - 1, ni = (p - 1) * (p - 2) / 2, nd = nd_of(p);
  const int64_t ndofs = (int64_t)m.nnodes + (int64_t)m.nfacets * ne + (int64_t)m.ncells * ni;
  if (ndofs > INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: %lld DOFs do not fit 32 bits", who, (long long)ndofs);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const size_t n = (size_t)m.ncells * nd;
  const bool host = memspace == EQLB_MEM_HOST;
  HostCall s; // (a device-memory call stages nothing: no allocation, no copy and no wait)
  const auto staged = s.out(host ? cell_dofs : nullptr, n);
  if (host)
    HIP_TRY(s.upload(stream));
  hipLaunchKernelGGL(k_lagrange_dofmap, dim3(grid_of(m.ncells, TR_THREADS)), dim3(TR_THREADS), 0, stream, m.ncells,
                     m.nnodes, m.nfacets, (int)p, m.cell_nodes, m.cell_facets, m.facet_perm,
                     host ? staged.get() : cell_dofs);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  if (ndofs_out)
    *ndofs_out = ndofs;
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_get_prolong_table(int32_t q, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (q < 1 || q > TR_PMAX || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_prolong_table: q = %d outside 1 ... 4, or null output", (int)q);
  const int n = (2 * q + 1) * (q + 1) * nd_of(q);
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_prolong_table: capacity too small");
  const double* t = q == 1 ? eqlb_tables::Prolong<1>::PT
                           : q == 2 ? eqlb_tables::Prolong<2>::PT
                                    : q == 3 ? eqlb_tables::Prolong<3>::PT : eqlb_tables::Prolong<4>::PT;
  for (int i = 0; i < n; ++i)
    out[i] = t[i];
  return n;
}

int eqlb_refine_prolong_lagrange(eqlb_refine_t* plan, eqlb_mesh_t* refined, int32_t p, int32_t bs, int32_t nrhs,
                                 const int32_t* cell_dofs, int64_t ndofs, const double* u, const int32_t* cell_dofs2,
                                 int64_t ndofs2, double* u2, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_refine_prolong_lagrange";
  if (!plan || !refined || !cell_dofs || !u || !cell_dofs2 || !u2)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (p < 1 || p > TR_PMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: p = %d outside 1 ... 4", who, (int)p);
  if (ndofs < 1 || ndofs > INT32_MAX || ndofs2 < 1 || ndofs2 > INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: ndofs = %lld, ndofs2 = %lld outside 1 ... 2^31 - 1", who,
                (long long)ndofs, (long long)ndofs2);
  ProlongArgs a;
  EQLB_TRY(common_args(who, plan, refined, bs, nrhs, memspace, a));
  // a handle of eqlb_mesh_create keeps node -> cell on the host until somebody needs it on the device
  if (mesh_node_cells(refined, &a.node_cells2))
    return EQLB_ERR_DEVICE;
  a.ndofs = ndofs;
  a.ndofs2 = ndofs2;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const int nd = nd_of(p);
  if (memspace == EQLB_MEM_DEVICE)
  {
    a.cell_dofs = cell_dofs;
    a.cell_dofs2 = cell_dofs2;
    a.in = u;
    a.out = u2;
    launch_prolong<false>(p, a, stream);
    HIP_TRY(hipGetLastError());
    return EQLB_OK;
  }
  // host memory: bad tables are caught here, before anything is launched
  const size_t n1 = (size_t)plan->ncells * nd, n2 = (size_t)plan->ncells2 * nd;
  const size_t nu = (size_t)nrhs * ndofs * bs, nu2 = (size_t)nrhs * ndofs2 * bs;
  EQLB_TRY(check_dofmap(who, "cell_dofs", cell_dofs, (size_t)plan->ncells, nd, ndofs));
  EQLB_TRY(check_dofmap(who, "cell_dofs2", cell_dofs2, (size_t)plan->ncells2, nd, ndofs2));
  HostCall s;
  const auto d_cd = s.in(cell_dofs, n1), d_cd2 = s.in(cell_dofs2, n2);
  const auto d_u = s.in(u, nu);
  // (entries that no DOF of cell_dofs2 names keep what the caller had there)
  const auto d_u2 = s.in(static_cast<const double*>(u2), nu2);
  s.out_prefix(u2, d_u2, nu2);
  HIP_TRY(s.upload(stream));
  a.cell_dofs = d_cd;
  a.cell_dofs2 = d_cd2;
  a.in = d_u;
  a.out = d_u2;
  launch_prolong<false>(p, a, stream);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_refine_prolong_dg(eqlb_refine_t* plan, eqlb_mesh_t* refined, int32_t degree, int32_t bs, int32_t nrhs,
                           const double* in, double* out, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_refine_prolong_dg";
  if (!plan || !refined || !in || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  if (degree < 0 || degree > TR_DMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: degree = %d outside 0 ... 3", who, (int)degree);
  ProlongArgs a;
  EQLB_TRY(common_args(who, plan, refined, bs, nrhs, memspace, a));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const size_t row = (size_t)nd_of(degree) * bs;
  const size_t n1 = (size_t)nrhs * plan->ncells * row, n2 = (size_t)nrhs * plan->ncells2 * row;
  const bool host = memspace == EQLB_MEM_HOST;
  HostCall s; // (a device-memory call stages nothing: no allocation, no copy and no wait)
  const auto d_in = s.in(host ? in : nullptr, n1);
  const auto d_out = s.out(host ? out : nullptr, n2);
  if (host)
    HIP_TRY(s.upload(stream));
  a.in = host ? d_in.get() : in;
  a.out = host ? d_out.get() : out;
  if (degree == 0)
    hipLaunchKernelGGL(k_prolong_dg0, dim3(grid_of(a.ncells, TR_THREADS)), dim3(TR_THREADS), 0, stream, a);
  else
    launch_prolong<true>(degree, a, stream);
  s.note(hipGetLastError());
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

} // extern "C"
