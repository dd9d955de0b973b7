// The P_p^2 linear-elasticity problem -div(2 eps(u) + pi_1 div(u) I) = f ON THE DEVICE: the counterpart of
// eqlb_primal_solve.hip for the displacement eqlb_primal_stress_dg takes - the primal solve of the reference's
// demo/elasticity_adaptive/demo_cook.py, which no DOLFINx can do on a mesh that was refined on the device.  The space is
// the scalar numbering of eqlb_mesh_lagrange_dofmap, blocked: u[2 dof + r].  The rule is stated in include/eqlb.h and,
// as numpy, in dolfinx_eqlb_amd/lsolver/primal.py (ElasticityOperator); operator, load, diagonal and residual
// reproduce the numpy statement bit for bit.
//
// The rule of a cell (no fused multiply-add anywhere; K = J^-1 as eqlb_primal_solve.hip forms it, K[X][d]):
//   Q[a][b][X][Y] = K[X][a] K[Y][b]
//   g_XY^s[i] = sum_j M_XY[i][j] u_s[j], ascending j, every product rounded on its own, with M_00 = S0 = Stiff<P>[0],
//               M_01 = Cross<P>, M_10 = Cross<P>^T, M_11 = S2 = Stiff<P>[2]
//   D_ab^s[i] = (Q[a][b][0][0] g_00^s[i] + Q[a][b][0][1] g_01^s[i]) + (Q[a][b][1][0] g_10^s[i] + Q[a][b][1][1] g_11^s[i])
//   y_loc[c][i][0] = |det J| (((D_00^0 + D_11^0) + (D_00^0 + D_10^1)) + pi_c (D_00^0 + D_01^1))
//   y_loc[c][i][1] = |det J| (((D_00^1 + D_11^1) + (D_01^0 + D_11^1)) + pi_c (D_10^0 + D_11^1))
//   diagonal (i, r): g_XY = M_XY[i][i], D_ab as above, |det J| (((D_00 + D_11) + D_rr) + pi_c D_rr)
//   load (i, r):     |det J| sum_n Load<P, D>[i][n] f_r[c][n], ascending n
//
//  k_elast_cell<P, MODE, D>  one thread per cell, ES_THREADS = 128 cells per workgroup: the 2 nd_p output values of a
//    cell are staged in LDS as k_primal_cell stages its nd_p, and at P = 4 the rows of 256 cells (62 KB) and the tables
//    would not fit a static block; 128 cells need 31 KB + 5.4 KB.  The tables (S0, S2, Cross: 3 nd_p^2 doubles; or
//    Load<P, D>) are read as a broadcast, the index rows of the workgroup move through LDS as one contiguous piece, and
//    so do the output rows y_loc [ncells][nd_p][2].
//  k_primal_gather<2, 1>, k_pcg_*<1>, pcg_solve: eqlb_primal_common.h, on one column of n = 2 ndofs rows with the
//    mask per row.
#include "eqlb_device_common.h"
#include "eqlb_mesh_handle.h" // (eqlb_host_util.h)
#include "eqlb_primal_common.h"
#include "eqlb_tables_gen.h"

#include <climits>
#include <cmath>

namespace eqlb
{
namespace
{
constexpr int ES_THREADS = 128; // cells per workgroup of the cell kernel

struct ElastCellArgs
{
  int32_t ncells;
  const int32_t* cell_dofs; // [ncells][nd_p], the scalar numbering
  const double *cellJ, *cell_pi1;
  double pi_1;
  const double* u;      // operator: [2 ndofs] blocked; load: rhs_dg [2][ncells][nd_d]
  const uint8_t* fixed; // [2 ndofs]; operator, only_fixed: the free rows of u read as 0
  int32_t only_fixed;
  double* yloc; // [ncells][nd_p][2]
  const PcgState* st;
};

template <int P, int MODE, int D>
__global__ void __launch_bounds__(ES_THREADS) k_elast_cell(const ElastCellArgs a)
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  constexpr int NP = nd_of(P), ND = nd_of(D), W = 2 * NP, S = W | 1, NN = NP * NP;
  constexpr int NTAB = (MODE == CELL_LOAD) ? NP * ND : 3 * NN;
  static_assert(eqlb_tables::Stiff<P>::ND == NP && eqlb_tables::Cross<P>::ND == NP && eqlb_tables::Load<P, D>::NP == NP
                    && eqlb_tables::Load<P, D>::ND == ND,
                "table shape");
  __shared__ double sT[NTAB];
  __shared__ double sbuf[ES_THREADS * S]; // first the index rows of the workgroup, then its output rows
  if (a.st && a.st->done)
    return;
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * ES_THREADS;
  const int nloc = (a.ncells - base < ES_THREADS) ? (int)(a.ncells - base) : ES_THREADS;
  const bool active = t < nloc;
  for (int i = t; i < NTAB; i += ES_THREADS)
  {
    if constexpr (MODE == CELL_LOAD)
      sT[i] = eqlb_tables::Load<P, D>::LD[i];
    else // S0 | S2 | Cross
      sT[i] = i < NN ? eqlb_tables::Stiff<P>::ST[i]
                     : i < 2 * NN ? eqlb_tables::Stiff<P>::ST[NN + i] : eqlb_tables::Cross<P>::CR[i - 2 * NN];
  }
  [[maybe_unused]] int32_t idx[NP];
  if constexpr (MODE == CELL_OPERATOR)
  {
    int32_t* sidx = reinterpret_cast<int32_t*>(sbuf);
    const int32_t* rows = a.cell_dofs + base * NP;
    for (int e = t; e < nloc * NP; e += ES_THREADS)
      sidx[e] = rows[e];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; ++i)
      idx[i] = active ? sidx[t * NP + i] : 0;
  }
  __syncthreads(); // the table is staged; the index rows are in registers: sbuf takes the output rows
  if (active)
  {
    const double2* Jp = reinterpret_cast<const double2*>(a.cellJ + 4 * (base + t));
    const double2 r0 = Jp[0], r1 = Jp[1]; // J00 J01 | J10 J11
    const double det = r0.x * r1.y - r0.y * r1.x;
    const double adet = fabs(det);
    if constexpr (MODE == CELL_LOAD)
    {
#pragma unroll
      for (int r = 0; r < 2; ++r)
      {
        const double* f = a.u + ((int64_t)r * a.ncells + base + t) * ND;
        double fv[ND];
#pragma unroll
        for (int n = 0; n < ND; ++n)
          fv[n] = f[n];
#pragma unroll
        for (int i = 0; i < NP; ++i)
        {
          double s = sT[i * ND] * fv[0];
#pragma unroll
          for (int n = 1; n < ND; ++n)
            s = s + sT[i * ND + n] * fv[n];
          sbuf[t * S + 2 * i + r] = adet * s;
        }
      }
    }
    else
    {
      const double idet = 1.0 / det;
      const double K[2][2] = {{r1.y * idet, -r0.y * idet}, {-r1.x * idet, r0.x * idet}}; // K[X][d]
      double Q[2][2][4];
#pragma unroll
      for (int aa = 0; aa < 2; ++aa)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
          for (int X = 0; X < 2; ++X)
#pragma unroll
            for (int Y = 0; Y < 2; ++Y)
              Q[aa][bb][2 * X + Y] = K[X][aa] * K[Y][bb];
      const double pi = a.cell_pi1 ? a.cell_pi1[base + t] : a.pi_1;
      [[maybe_unused]] double uu[2][NP];
      if constexpr (MODE == CELL_OPERATOR)
      {
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
          for (int r = 0; r < 2; ++r)
          {
            const int64_t e = 2 * (int64_t)idx[i] + r;
            const double v = a.u[e];
            uu[r][i] = (a.only_fixed && !a.fixed[e]) ? 0.0 : v;
          }
      }
      const double *S0 = sT, *S2 = sT + NN, *CR = sT + 2 * NN;
      // the rows are a loop from P = 3 on: unrolled, the compiler keeps table values of many rows in flight and P = 4
      // takes 256 VGPRs + 238 AGPRs; i indexes LDS only, so the loop needs no register array indexed by it
      constexpr int UNROLL_ROWS = NP <= 6 ? NP : 1;
#pragma unroll UNROLL_ROWS
      for (int i = 0; i < NP; ++i)
      {
        if constexpr (MODE == CELL_DIAGONAL)
        {
          const double g[4] = {S0[i * NP + i], CR[i * NP + i], CR[i * NP + i], S2[i * NP + i]};
          double Dd[2][2];
#pragma unroll
          for (int aa = 0; aa < 2; ++aa)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
              Dd[aa][bb] = (Q[aa][bb][0] * g[0] + Q[aa][bb][1] * g[1]) + (Q[aa][bb][2] * g[2] + Q[aa][bb][3] * g[3]);
#pragma unroll
          for (int r = 0; r < 2; ++r)
            sbuf[t * S + 2 * i + r] = adet * (((Dd[0][0] + Dd[1][1]) + Dd[r][r]) + pi * Dd[r][r]);
        }
        else
        {
          double Dd[2][2][2]; // [s][a][b]
#pragma unroll
          for (int s = 0; s < 2; ++s)
          {
            double g0 = S0[i * NP] * uu[s][0], g1 = CR[i * NP] * uu[s][0], g2 = CR[i] * uu[s][0],
                   g3 = S2[i * NP] * uu[s][0];
#pragma unroll
            for (int j = 1; j < NP; ++j)
            {
              g0 = g0 + S0[i * NP + j] * uu[s][j];
              g1 = g1 + CR[i * NP + j] * uu[s][j];
              g2 = g2 + CR[j * NP + i] * uu[s][j];
              g3 = g3 + S2[i * NP + j] * uu[s][j];
            }
#pragma unroll
            for (int aa = 0; aa < 2; ++aa)
#pragma unroll
              for (int bb = 0; bb < 2; ++bb)
                Dd[s][aa][bb] = (Q[aa][bb][0] * g0 + Q[aa][bb][1] * g1) + (Q[aa][bb][2] * g2 + Q[aa][bb][3] * g3);
          }
          sbuf[t * S + 2 * i] = adet * (((Dd[0][0][0] + Dd[0][1][1]) + (Dd[0][0][0] + Dd[1][1][0]))
                                        + pi * (Dd[0][0][0] + Dd[1][0][1]));
          sbuf[t * S + 2 * i + 1] = adet * (((Dd[1][0][0] + Dd[1][1][1]) + (Dd[0][0][1] + Dd[1][1][1]))
                                            + pi * (Dd[0][1][0] + Dd[1][1][1]));
        }
      }
    }
  }
  __syncthreads();
  double* o = a.yloc + base * W;
  for (int e = t; e < nloc * W; e += ES_THREADS)
    o[e] = sbuf[(e / W) * S + (e % W)];
}

// the mask of component r: the rows 2 dof + r of the vertex and facet DOFs of the listed facets; ids outside the mesh are
// skipped and counted (status[0]), valid ones counted per component (status[1 + r])
__global__ void __launch_bounds__(PS_THREADS)
k_elast_mask(int32_t nlist, const int32_t* __restrict__ facets, int32_t r, int32_t nnodes, int32_t nfacets, int32_t ne,
             const int32_t* __restrict__ facet_nodes, uint8_t* __restrict__ fixed, int32_t* __restrict__ status)
{
  const int32_t i = blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= nlist)
    return;
  const int32_t f = facets[i];
  if (f < 0 || f >= nfacets)
  {
    atomicAdd(status, 1);
    return;
  }
  atomicAdd(status + 1 + r, 1);
  fixed[2 * (int64_t)facet_nodes[2 * (int64_t)f] + r] = 1;
  fixed[2 * (int64_t)facet_nodes[2 * (int64_t)f + 1] + r] = 1;
  for (int j = 0; j < ne; ++j)
    fixed[2 * ((int64_t)nnodes + (int64_t)f * ne + j) + r] = 1;
}

// ---- host side ------------------------------------------------------------------------------------------------
template <int P, int MODE>
hipError_t launch_cell_d(int d, const ElastCellArgs& a, hipStream_t stream)
{
  const dim3 grid(grid_of(a.ncells, ES_THREADS)), block(ES_THREADS);
  if constexpr (MODE != CELL_LOAD)
    hipLaunchKernelGGL((k_elast_cell<P, MODE, 0>), grid, block, 0, stream, a);
  else
    switch (d)
    {
    case 0:
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 0>), grid, block, 0, stream, a);
      break;
    case 1:
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 1>), grid, block, 0, stream, a);
      break;
    case 2:
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 2>), grid, block, 0, stream, a);
      break;
    default:
      hipLaunchKernelGGL((k_elast_cell<P, MODE, 3>), grid, block, 0, stream, a);
    }
  return hipGetLastError();
}

template <int MODE>
hipError_t launch_cell(int p, int d, const ElastCellArgs& a, hipStream_t stream)
{
  switch (p)
  {
  case 1:
    return launch_cell_d<1, MODE>(d, a, stream);
  case 2:
    return launch_cell_d<2, MODE>(d, a, stream);
  case 3:
    return launch_cell_d<3, MODE>(d, a, stream);
  default:
    return launch_cell_d<4, MODE>(d, a, stream);
  }
}
} // namespace
} // namespace eqlb

// the handle behind eqlb_elasticity_t: everything is carved out of one allocation at create
struct eqlb_elasticity
{
  eqlb_mesh* mesh = nullptr;
  int p = 0, nd = 0;
  int64_t ndofs = 0; // scalar; the vectors have 2 ndofs rows
  bool has_pi1 = false;
  double pi_1 = 1.0;
  eqlb::SpaceArgs space{};
  eqlb::DevCarve mem;
  // status: skipped facet ids, listed valid ones of component 0, of component 1, unmatched slots
  eqlb::DevPiece<int32_t> cell_dofs, slots, status;
  eqlb::DevPiece<double> cell_pi1, yloc, diag, r, z, d, q, part;
  eqlb::DevPiece<uint8_t> fixed;
  eqlb::DevPiece<eqlb::PcgState> st;
};

namespace eqlb
{
namespace
{
const ManyCols ONE_COLUMN{1, 1u, 0, nullptr}; // a launch that knows no state (the handle has one column)

ElastCellArgs cell_args(const eqlb_elasticity& h, const ManyCols& c, const double* u, bool only_fixed)
{
  ElastCellArgs a{};
  a.ncells = h.space.ncells;
  a.cell_dofs = h.cell_dofs;
  a.cellJ = h.mesh->m.cellJ;
  a.cell_pi1 = h.has_pi1 ? h.cell_pi1.get() : nullptr;
  a.pi_1 = h.pi_1;
  a.u = u;
  a.fixed = h.fixed;
  a.only_fixed = only_fixed ? 1 : 0;
  a.yloc = h.yloc;
  a.st = c.check ? c.st : nullptr;
  return a;
}

GatherArgs gather_args(const eqlb_elasticity& h, const ManyCols& c, bool masked)
{
  GatherArgs g{};
  g.s = h.space;
  g.yloc = h.yloc;
  g.fixed = masked ? h.fixed.get() : nullptr;
  g.part = h.part;
  g.cols = c;
  return g;
}

hipError_t launch_gather(const eqlb_elasticity& h, const GatherArgs& g, hipStream_t stream)
{
  hipLaunchKernelGGL((k_primal_gather<2, 1>), dim3(stream_blocks(2 * h.ndofs)), dim3(PS_THREADS), 0, stream, g);
  return hipGetLastError();
}

PcgWork pcg_work(const eqlb_elasticity& h)
{
  return PcgWork{2 * h.ndofs, 1, h.diag, h.fixed, h.yloc, h.r, h.z, h.d, h.q, h.part, h.st};
}

// y = owner sum of y_loc (masked or raw); y DEVICE
hipError_t enqueue_owner_sum(const eqlb_elasticity& h, const ManyCols& c, double* y, bool masked, hipStream_t stream)
{
  GatherArgs g = gather_args(h, c, masked);
  g.y = y;
  return launch_gather(h, g, stream);
}

// y = A u (masked or raw); all pointers DEVICE
hipError_t enqueue_apply(const eqlb_elasticity& h, const double* u, double* y, bool masked, hipStream_t stream)
{
  const hipError_t e = launch_cell<CELL_OPERATOR>(h.p, 0, cell_args(h, ONE_COLUMN, u, false), stream);
  return e != hipSuccess ? e : enqueue_owner_sum(h, ONE_COLUMN, y, masked, stream);
}

hipError_t enqueue_diagonal(const eqlb_elasticity& h, double* out, hipStream_t stream)
{
  const hipError_t e = launch_cell<CELL_DIAGONAL>(h.p, 0, cell_args(h, ONE_COLUMN, nullptr, false), stream);
  return e != hipSuccess ? e : enqueue_owner_sum(h, ONE_COLUMN, out, false, stream);
}

// r = b - A u (0 on the fixed rows), u^ instead of u with only_fixed; the block partials of r.r are left in h.part
hipError_t enqueue_residual(const eqlb_elasticity& h, const ManyCols& c, const double* b, const double* u, double* r,
                            bool only_fixed, hipStream_t stream)
{
  const hipError_t e = launch_cell<CELL_OPERATOR>(h.p, 0, cell_args(h, c, u, only_fixed), stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, c, true);
  g.b = b;
  g.r = r;
  g.dot = DOT_R_R;
  return launch_gather(h, g, stream);
}

// q = A d on the free rows (the direction d of the handle), the block partials of d.q in h.part
hipError_t enqueue_product(const eqlb_elasticity& h, const ManyCols& c, hipStream_t stream)
{
  const hipError_t e = launch_cell<CELL_OPERATOR>(h.p, 0, cell_args(h, c, h.d, false), stream);
  if (e != hipSuccess)
    return e;
  GatherArgs g = gather_args(h, c, true);
  g.y = h.q;
  g.w = h.d;
  g.dot = DOT_W_Y;
  return launch_gather(h, g, stream);
}

int check_handle(const char* who, const eqlb_elasticity* h)
{
  if (!h)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null handle", who);
  return EQLB_OK;
}
} // namespace

// the handle as the hierarchy unit sees it (eqlb_internal.h: SolverLevel)
void elasticity_level(eqlb_elasticity* h, SolverLevel& v)
{
  v = SolverLevel{};
  v.handle = h;
  v.mesh = h->mesh;
  v.p = h->p;
  v.bs = 2;
  v.ndofs = h->ndofs;
  v.cell_dofs = h->cell_dofs;
  v.diag = h->diag;
  v.fixed = h->fixed;
  v.status = h->status;
  v.work = [](void* hh, int R, PcgWork& w) {
    if (R != 1)
      return fail(EQLB_ERR_UNSUPPORTED,
                  "elasticity_level: several right-hand sides are provided for Poisson handles (bs = 1) only");
    w = pcg_work(*static_cast<eqlb_elasticity*>(hh));
    return (int)EQLB_OK;
  };
  v.owner_sum = [](void* hh, const ManyCols& c, double* y, bool masked, hipStream_t stream) {
    return enqueue_owner_sum(*static_cast<eqlb_elasticity*>(hh), c, y, masked, stream);
  };
  v.residual = [](void* hh, const ManyCols& c, const double* b, const double* u, double* r, bool only_fixed,
                  hipStream_t stream) {
    return enqueue_residual(*static_cast<eqlb_elasticity*>(hh), c, b, u, r, only_fixed, stream);
  };
  v.product = [](void* hh, const ManyCols& c, hipStream_t stream) {
    return enqueue_product(*static_cast<eqlb_elasticity*>(hh), c, stream);
  };
}
} // namespace eqlb

extern "C" {

int eqlb_get_cross_table(int32_t p, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (p < 1 || p > PS_PMAX || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_cross_table: p = %d outside 1 ... 4, or null output", (int)p);
  const int n = nd_of(p) * nd_of(p);
  if (capacity < n)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_cross_table: capacity too small");
  const double* t = p == 1 ? eqlb_tables::Cross<1>::CR
                           : p == 2 ? eqlb_tables::Cross<2>::CR
                                    : p == 3 ? eqlb_tables::Cross<3>::CR : eqlb_tables::Cross<4>::CR;
  for (int i = 0; i < n; ++i)
    out[i] = t[i];
  return n;
}

int eqlb_elasticity_create(eqlb_mesh_t* mesh, int32_t p, double pi_1, const double* cell_pi1, int32_t memspace,
                           void* stream_, eqlb_elasticity_t** handle)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_elasticity_create";
  if (p < 1 || p > PS_PMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: p = %d outside 1 ... 4", who, (int)p);
  if (!mesh || !handle)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  const DeviceMesh& m = mesh->m;
  const int ne = p - 1, ni = (p - 1) * (p - 2) / 2, nd = nd_of(p);
  const int64_t ndofs = (int64_t)m.nnodes + (int64_t)m.nfacets * ne + (int64_t)m.ncells * ni;
  if (ndofs > INT32_MAX || (int64_t)m.ncells * nd > INT32_MAX || m.ncells < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: %lld DOFs, %lld cell entries do not fit 32 bits", who, (long long)ndofs,
                (long long)m.ncells * nd);
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  // a handle of eqlb_mesh_create keeps node -> cell on the host until somebody needs it on the device
  const int32_t* node_cells = nullptr;
  if (mesh_node_cells(mesh, &node_cells))
    return EQLB_ERR_DEVICE;
  std::unique_ptr<eqlb_elasticity> h(new eqlb_elasticity);
  h->mesh = mesh;
  h->p = p;
  h->nd = nd;
  h->ndofs = ndofs;
  h->has_pi1 = cell_pi1 != nullptr;
  h->pi_1 = pi_1;
  const size_t nc = (size_t)m.ncells, nslots = 3 * nc * (size_t)(1 + ne), nv = 2 * (size_t)ndofs;
  h->cell_dofs = h->mem.piece<int32_t>(nc * nd);
  h->slots = h->mem.piece<int32_t>(nslots);
  h->status = h->mem.piece<int32_t>(4);
  h->cell_pi1 = h->mem.piece<double>(nc);
  h->yloc = h->mem.piece<double>(2 * nc * nd);
  h->diag = h->mem.piece<double>(nv);
  h->r = h->mem.piece<double>(nv);
  h->z = h->mem.piece<double>(nv);
  h->d = h->mem.piece<double>(nv);
  h->q = h->mem.piece<double>(nv);
  h->part = h->mem.piece<double>(2 * (size_t)PS_MAXBLOCKS);
  h->fixed = h->mem.piece<uint8_t>(nv);
  h->st = h->mem.piece<PcgState>(1);
  HIP_TRY(h->mem.alloc());
  SpaceArgs& s = h->space;
  s.ndofs = ndofs;
  s.nnodes = m.nnodes;
  s.nfacets = m.nfacets;
  s.ncells = m.ncells;
  s.ne = ne;
  s.ni = ni > 0 ? ni : 1;
  s.nd = nd;
  s.nco = m.node_cells_off;
  s.fco = m.facet_cells_off;
  s.slots = h->slots;
  HIP_TRY(hipMemsetAsync(h->status, 0, 4 * sizeof(int32_t), stream));
  HIP_TRY(hipMemsetAsync(h->fixed, 0, nv, stream));
  if (cell_pi1)
    HIP_TRY(hipMemcpyAsync(h->cell_pi1, cell_pi1, nc * sizeof(double),
                           memspace == EQLB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
  // the dofmap, by the kernel behind eqlb_mesh_lagrange_dofmap (device memory space: one launch, nothing waits)
  EQLB_TRY(eqlb_mesh_lagrange_dofmap(mesh, p, h->cell_dofs.get(), nullptr, EQLB_MEM_DEVICE, stream_));
  const int64_t nshared = (int64_t)m.nnodes + (int64_t)m.nfacets * ne;
  // (k_primal_slots counts an unmatched slot in the third word behind its status pointer: status[3] here)
  hipLaunchKernelGGL(k_primal_slots, dim3(grid_of(nshared, PS_THREADS)), dim3(PS_THREADS), 0, stream, s, node_cells,
                     m.facet_cells, h->cell_dofs.get(), h->slots.get(), h->status.get() + 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(enqueue_diagonal(*h, h->diag, stream));
  if (memspace == EQLB_MEM_HOST)
    HIP_TRY(hipStreamSynchronize(stream)); // (the caller's array has been read)
  *handle = h.release();
  return EQLB_OK;
}
EQLB_CATCH_ALL

void eqlb_elasticity_destroy(eqlb_elasticity_t* handle) { delete handle; }

int eqlb_elasticity_ndofs(const eqlb_elasticity_t* handle, int64_t* ndofs)
{
  using namespace eqlb;
  if (!handle || !ndofs)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_elasticity_ndofs: null argument");
  *ndofs = handle->ndofs;
  return EQLB_OK;
}

int eqlb_elasticity_set_dirichlet(eqlb_elasticity_t* h, int32_t nlist0, const int32_t* facets0, int32_t nlist1,
                                  const int32_t* facets1, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_elasticity_set_dirichlet";
  const int32_t nlist[2] = {nlist0, nlist1};
  const int32_t* const facets[2] = {facets0, facets1};
  for (int r = 0; r < 2; ++r)
    if (nlist[r] < 0 || (nlist[r] > 0 && !facets[r]))
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nlist%d = %d, or a null list", who, r, (int)nlist[r]);
  EQLB_TRY(check_handle(who, h));
  EQLB_TRY(check_memspace(who, memspace));
  const DeviceMesh& m = h->mesh->m;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  if (host)
    for (int r = 0; r < 2; ++r)
      for (int32_t i = 0; i < nlist[r]; ++i)
        if (facets[r][i] < 0 || facets[r][i] >= m.nfacets)
          return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: facets%d[%d] = %d is no facet of the mesh (%d facets)", who, r,
                      (int)i, (int)facets[r][i], (int)m.nfacets);
  HostCall s; // (a device-memory call stages nothing: no allocation, no copy and no wait)
  const DevPiece<int32_t> d_f[2] = {s.in(host ? facets0 : nullptr, (size_t)nlist0),
                                    s.in(host ? facets1 : nullptr, (size_t)nlist1)};
  if (host && (nlist0 > 0 || nlist1 > 0))
    HIP_TRY(s.upload(stream));
  s.note(hipMemsetAsync(h->fixed, 0, 2 * (size_t)h->ndofs, stream));
  s.note(hipMemsetAsync(h->status, 0, 3 * sizeof(int32_t), stream));
  for (int r = 0; r < 2; ++r)
    if (nlist[r] > 0)
    {
      hipLaunchKernelGGL(k_elast_mask, dim3(grid_of(nlist[r], PS_THREADS)), dim3(PS_THREADS), 0, stream, nlist[r],
                         host ? d_f[r].get() : facets[r], r, m.nnodes, m.nfacets, h->space.ne, m.facet_nodes,
                         h->fixed.get(), h->status.get());
      s.note(hipGetLastError());
    }
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_elasticity_load(eqlb_elasticity_t* h, int32_t degree_dg, const double* rhs_dg, const double* b_extra,
                         double* b, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_elasticity_load";
  if (degree_dg < 0 || degree_dg > PS_DMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: degree_dg = %d outside 0 ... 3", who, (int)degree_dg);
  EQLB_TRY(check_handle(who, h));
  if (!rhs_dg || !b)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t nf = 2 * (size_t)h->space.ncells * nd_of(degree_dg), n = 2 * (size_t)h->ndofs;
  HostCall s;
  const auto d_f = s.in(host ? rhs_dg : nullptr, nf), d_e = s.in(host ? b_extra : nullptr, n);
  const auto d_b = s.out(host ? b : nullptr, n);
  if (host)
    HIP_TRY(s.upload(stream));
  s.note(launch_cell<CELL_LOAD>(h->p, degree_dg, cell_args(*h, ONE_COLUMN, host ? d_f.get() : rhs_dg, false), stream));
  GatherArgs g = gather_args(*h, ONE_COLUMN, false);
  g.add = host ? d_e.get() : b_extra;
  g.y = host ? d_b.get() : b;
  s.note(launch_gather(*h, g, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_elasticity_apply(eqlb_elasticity_t* h, const double* u, double* y, int32_t masked, int32_t memspace,
                          void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_elasticity_apply";
  EQLB_TRY(check_handle(who, h));
  if (!u || !y)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = 2 * (size_t)h->ndofs;
  HostCall s;
  const auto d_u = s.in(host ? u : nullptr, n);
  const auto d_y = s.out(host ? y : nullptr, n);
  if (host)
    HIP_TRY(s.upload(stream));
  s.note(enqueue_apply(*h, host ? d_u.get() : u, host ? d_y.get() : y, masked != 0, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_elasticity_diagonal(eqlb_elasticity_t* h, double* out, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_elasticity_diagonal";
  EQLB_TRY(check_handle(who, h));
  if (!out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  HostCall s;
  const auto d_o = s.out(host ? out : nullptr, 2 * (size_t)h->ndofs);
  if (host)
    HIP_TRY(s.upload(stream));
  s.note(enqueue_diagonal(*h, host ? d_o.get() : out, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_elasticity_residual(eqlb_elasticity_t* h, const double* b, const double* u, double* r, double* norms,
                             int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_elasticity_residual";
  EQLB_TRY(check_handle(who, h));
  if (!b || !u || !r)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const bool host = memspace == EQLB_MEM_HOST;
  const size_t n = 2 * (size_t)h->ndofs;
  HostCall s;
  const auto d_b = s.in(host ? b : nullptr, n), d_u = s.in(host ? u : nullptr, n);
  const auto d_r = s.out(host ? r : nullptr, n);
  const auto d_n = s.out(host ? norms : nullptr, 2);
  if (host)
    HIP_TRY(s.upload(stream));
  const double *pb = host ? d_b.get() : b, *pu = host ? d_u.get() : u;
  double* pn = host ? d_n.get() : norms;
  if (pn)
  {
    // the reference norm first, into the work vector q: the residual proper then leaves r as the caller sees it
    s.note(enqueue_residual(*h, ONE_COLUMN, pb, pu, h->q, true, stream));
    s.note(launch_scalar(pcg_work(*h), 1u, STEP_NORM, 0, 0.0, 0.0, pn + 1, stream));
  }
  s.note(enqueue_residual(*h, ONE_COLUMN, pb, pu, host ? d_r.get() : r, false, stream));
  if (pn)
    s.note(launch_scalar(pcg_work(*h), 1u, STEP_NORM, 0, 0.0, 0.0, pn, stream));
  HIP_TRY(s.finish(stream));
  return EQLB_OK;
}
EQLB_CATCH_ALL

int eqlb_elasticity_solve(eqlb_elasticity_t* h, const double* b, double* u, double rtol, double atol, int32_t maxit,
                          double* info, int32_t memspace, void* stream_)
try
{
  using namespace eqlb;
  const char* const who = "eqlb_elasticity_solve";
  if (maxit < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: maxit = %d (at least 1)", who, (int)maxit);
  if (!(rtol >= 0.0) || !(atol >= 0.0))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: rtol = %g, atol = %g negative or NaN", who, rtol, atol);
  EQLB_TRY(check_handle(who, h));
  if (!b || !u || !info)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  // the status word of the mask: the call waits by nature, and nothing is launched for a singular problem
  int32_t status[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, h->status.get(), sizeof(status), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int r = 0; r < 2; ++r)
    if (status[1 + r] < 1)
      return fail(EQLB_ERR_INVALID_ARGUMENT,
                  "%s: singular: component %d has no Dirichlet DOF (eqlb_elasticity_set_dirichlet first)", who, r);
  auto residual = [&](const ManyCols& c, const double* pb, const double* pu, double* r, bool only_fixed) {
    return enqueue_residual(*h, c, pb, pu, r, only_fixed, stream);
  };
  auto product = [&](const ManyCols& c) { return enqueue_product(*h, c, stream); };
  const PcgWork w = pcg_work(*h);
  return pcg_solve_groups(w.n, 1, b, u, info, memspace == EQLB_MEM_HOST, stream,
                          [&](int, const double* pb, double* pu, double* pinfo) {
                            return pcg_solve(w, residual, product, JacobiSteps<1>{w, stream}, pb, pu, rtol, atol, maxit,
                                             pinfo, status[0], stream);
                          });
}
EQLB_CATCH_ALL

} // extern "C"
