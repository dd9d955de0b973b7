// Projected flux / stress of a P_p primal solution on the device - the step in front of the equilibration that the
// reference writes in UFL: sigma_h = -grad(u_h), -k grad(u_h) with a cell-wise k (demo/poisson_adaptive/
// demo_discont-coeff.py), 2 eps(u_h) + pi_1 div(u_h) I (demo/elasticity_adaptive/demo_cook.py), handed to
// local_projection(V_flux_proj, [sigma_h]) (python/dolfinx_eqlb/lsolver/projection.py:17-77).
//
// Quadrature-free: on an affine cell grad u_h = K^T grad_X u_h with K = J^-1, and grad_X u_h lies in P_{p-1}^2 on the
// reference cell, so its DG_d DOFs are ONE constant matrix per (p, d) applied to the DOFs of the cell,
//   gref[n][X]    = sum_i PG<p,d>[X][n][i] u[cell_dofs[c][i]]        (tools/gen_tables.py: primal_table_exact)
//   flux_dg[c][n] = -kappa_c K_c^T gref[n]
// and for a displacement u = (u_0, u_1) with gu[r][d] = d_d u_r from the same gref per component:
//   sigma = gu + gu^T + pi_1 tr(gu) I,   output row r = -sigma[r][:].
//
// k_primal_flux<P, D, STRESS>: a streaming gather kernel, one thread per cell, PF_THREADS cells per workgroup.
//  - the index rows of the workgroup's cells are read as one contiguous piece and handed out through LDS, the table
//    (a kernel argument: built-in or the caller's `op`) is staged in LDS once;
//  - the 2 nd_d values of a cell are staged in LDS (row stride 2 nd_d + 1 doubles: an odd stride of 8-byte words, no
//    bank conflict of the thread-per-row writes) and written as the contiguous piece of flux_dg the workgroup owns;
//  - several right-hand sides reuse the index row, which stays in registers;
//  - every gathered index is checked against [0, ndofs): a cell with a bad index writes NaN and reads nothing there.
// The nd_p products of a contraction are rounded one by one, put in ascending order by a sorting network and added
// from the smallest up.  The sum then depends on the SET of products only: a caller's table `op` whose columns are
// permuted together with cell_dofs gives the same bits as the built-in one.  No atomics, no scratch, one fixed order
// of operations per value: two runs give the same bits.
#include "eqlb_device_common.h"
#include "eqlb_mesh_handle.h" // (eqlb_host_util.h)
#include "eqlb_tables_gen.h"
#include <cmath>
#include <cstring>

namespace eqlb
{

constexpr int PF_THREADS = 256;
constexpr int PF_PMAX = 4, PF_DMAX = 3;

template <int P, int D>
struct PrimalOp
{
  double v[2 * nd_of(D) * nd_of(P)]; // PG[X][n][i]
};

// Batcher's merge exchange for N keys (any N) as a list of compare-exchange pairs
template <int N>
struct SortNet
{
  int n;
  int a[N * N + 1], b[N * N + 1];
  constexpr SortNet() : n(0), a{}, b{}
  {
    for (int p = 1; p < N; p <<= 1)
      for (int k = p; k >= 1; k >>= 1)
        for (int j = k % p; j + k < N; j += 2 * k)
          for (int i = 0; i < k && i + j + k < N; ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p))
            {
              a[n] = i + j;
              b[n] = i + j + k;
              ++n;
            }
  }
};

// sum of t[0 .. N) that does not depend on their order: ascending by the network, then added from the smallest up
// (compare and select, not min / max: a NaN stays in the list and reaches the sum)
template <int N>
__device__ __forceinline__ double sorted_sum(double (&t)[N])
{
  constexpr SortNet<N> net{};
#pragma unroll
  for (int c = 0; c < net.n; ++c)
  {
    const double x = t[net.a[c]], y = t[net.b[c]];
    const bool sw = y < x;
    t[net.a[c]] = sw ? y : x;
    t[net.b[c]] = sw ? x : y;
  }
  double s = t[0];
#pragma unroll
  for (int i = 1; i < N; ++i)
    s = __dadd_rn(s, t[i]);
  return s;
}

// the shear modulus of eqlb_primal_stress_dg_mu: mu_T = cell_mu[cell] where given, else the scalar mu.  A kernel
// argument of its own, which k_primal_flux does not take.
struct StressMuArgs
{
  const double* cell_mu = nullptr; // [ncells] or nullptr
  double mu = 1.0;
};

// k_primal_flux<P, D, STRESS> and, from the same source (eqlb_primal_flux_kernel.inc), k_primal_stress_mu<P, D>: the
// stress with a cell-wise shear modulus, every output value mu_T times the value k_primal_flux<P, D, true> forms,
// rounded once.  A kernel of its own, so that eqlb_primal_flux_dg and eqlb_primal_stress_dg launch the symbols,
// arguments and code they launched before (tools/isa_compare.py).
// k_primal_flux_tensor<P, D>, the third variant: the flux -kappa_T D_T grad u_h of eqlb_primal_flux_dg_tensor with the
// symmetric tensor D_T = (d00, d01, d11) of the cell, one 2 x 2 product per DG coefficient on top of the gradient.
struct FluxTensorArgs
{
  const double* cell_D = nullptr; // [ncells][3]
};

#define EQLB_FLUX_TENSOR 0
#define EQLB_FLUX_MU 0
#include "eqlb_primal_flux_kernel.inc"
#undef EQLB_FLUX_MU
#define EQLB_FLUX_MU 1
#include "eqlb_primal_flux_kernel.inc"
#undef EQLB_FLUX_MU
#undef EQLB_FLUX_TENSOR
#define EQLB_FLUX_TENSOR 1
#define EQLB_FLUX_MU 0
#include "eqlb_primal_flux_kernel.inc"
#undef EQLB_FLUX_MU
#undef EQLB_FLUX_TENSOR

// The projected VALUE of a P_p function, the piece that turns c u_h into the right-hand side the equilibrator needs for
// an operator with a reaction term (rhs = Pi_d f - c_T Pi_d u_h):
//   out[r][c][n] = cell_coeff[c] sum_i PV<p,d>[n][i] u[r][cell_dofs[c][i]]
// ascending i, every product rounded on its own (a caller's `op` with permuted columns therefore gives other last bits:
// the statement is the ascending sum).  The launch shape, the staging through LDS and the index check are those of
// k_primal_flux; a row has nd_d values.
template <int P, int D>
struct ValueOp
{
  double v[nd_of(D) * nd_of(P)]; // PV[n][i]
};

template <int P, int D>
__global__ void __launch_bounds__(PF_THREADS)
k_primal_value(int32_t ncells, int32_t nrhs, int64_t ndofs, const int32_t* __restrict__ cell_dofs,
               const double* __restrict__ u, const double* __restrict__ coeff, const ValueOp<P, D> op,
               double* __restrict__ out)
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  constexpr int NP = nd_of(P), ND = nd_of(D), ROW = ND, S = ROW | 1;
  constexpr int NBUF = (PF_THREADS * S > (PF_THREADS * NP + 1) / 2) ? PF_THREADS * S : (PF_THREADS * NP + 1) / 2;
  __shared__ double sPV[ND * NP];
  __shared__ double sbuf[NBUF]; // first the index rows of the workgroup, then its output rows
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * PF_THREADS;
  const int nloc = (ncells - base < PF_THREADS) ? (int)(ncells - base) : PF_THREADS;
  const bool active = t < nloc;
  for (int i = t; i < ND * NP; i += PF_THREADS)
    sPV[i] = op.v[i];
  int32_t* sidx = reinterpret_cast<int32_t*>(sbuf);
  const int32_t* rows = cell_dofs + base * NP;
  for (int e = t; e < nloc * NP; e += PF_THREADS)
    sidx[e] = rows[e];
  __syncthreads();
  int32_t idx[NP];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NP; ++i)
  {
    idx[i] = active ? sidx[t * NP + i] : 0;
    ok = ok && idx[i] >= 0 && (int64_t)idx[i] < ndofs;
  }
  const bool scaled = coeff != nullptr;
  const double kap = (active && scaled) ? coeff[base + t] : 1.0;
  const double bad = __longlong_as_double(0x7ff8000000000000ll);
  __syncthreads(); // the index rows are in registers: sbuf takes the output rows
  for (int r = 0; r < nrhs; ++r)
  {
    if (active)
    {
      const double* ur = u + (int64_t)r * ndofs;
      double uu[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i)
        uu[i] = ok ? ur[idx[i]] : 0.0;
#pragma unroll
      for (int n = 0; n < ND; ++n)
      {
        double v = sPV[n * NP] * uu[0];
#pragma unroll
        for (int i = 1; i < NP; ++i)
          v = v + sPV[n * NP + i] * uu[i];
        if (scaled)
          v = kap * v;
        sbuf[t * S + n] = ok ? v : bad;
      }
    }
    __syncthreads();
    double* o = out + ((int64_t)r * ncells + base) * ROW;
    for (int e = t; e < nloc * ROW; e += PF_THREADS)
      o[e] = sbuf[(e / ROW) * S + (e % ROW)];
    __syncthreads();
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
template <int P, int D>
static void builtin_table(double* out)
{
  using T = eqlb_tables::Primal<P, D>;
  for (int i = 0; i < 2 * T::ND * T::NP; ++i)
    out[i] = T::PG[i];
}

template <int P, int D>
static hipError_t launch_pd(bool stress, int32_t ncells, int32_t nrhs, int64_t ndofs, const int32_t* cell_dofs,
                            const double* u, const double* cellJ, const double* coeff, double pi_1, const double* op,
                            double* out, const StressMuArgs* sx, const FluxTensorArgs* tx, hipStream_t stream)
{
  PrimalOp<P, D> tab;
  if (op)
    std::memcpy(tab.v, op, sizeof(tab.v));
  else
    builtin_table<P, D>(tab.v);
  const unsigned grid = (unsigned)(((int64_t)ncells + PF_THREADS - 1) / PF_THREADS);
  if (!stress && tx) // the variant with the diffusion tensor
    hipLaunchKernelGGL((k_primal_flux_tensor<P, D>), dim3(grid), dim3(PF_THREADS), 0, stream, ncells, nrhs, ndofs,
                       cell_dofs, u, cellJ, coeff, pi_1, tab, out, *tx);
  else if (stress && sx) // the variant with the shear modulus; without it the launch as before the term existed
    hipLaunchKernelGGL((k_primal_stress_mu<P, D>), dim3(grid), dim3(PF_THREADS), 0, stream, ncells, nrhs, ndofs, cell_dofs,
                       u, cellJ, coeff, pi_1, tab, out, *sx);
  else if (stress)
    hipLaunchKernelGGL((k_primal_flux<P, D, true>), dim3(grid), dim3(PF_THREADS), 0, stream, ncells, nrhs, ndofs,
                       cell_dofs, u, cellJ, coeff, pi_1, tab, out);
  else
    hipLaunchKernelGGL((k_primal_flux<P, D, false>), dim3(grid), dim3(PF_THREADS), 0, stream, ncells, nrhs, ndofs,
                       cell_dofs, u, cellJ, coeff, pi_1, tab, out);
  return hipGetLastError();
}

template <int P>
static hipError_t launch_p(int d, bool stress, int32_t ncells, int32_t nrhs, int64_t ndofs, const int32_t* cell_dofs,
                           const double* u, const double* cellJ, const double* coeff, double pi_1, const double* op,
                           double* out, const StressMuArgs* sx, const FluxTensorArgs* tx, hipStream_t stream)
{
  switch (d)
  {
  case 0:
    return launch_pd<P, 0>(stress, ncells, nrhs, ndofs, cell_dofs, u, cellJ, coeff, pi_1, op, out, sx, tx, stream);
  case 1:
    return launch_pd<P, 1>(stress, ncells, nrhs, ndofs, cell_dofs, u, cellJ, coeff, pi_1, op, out, sx, tx, stream);
  case 2:
    return launch_pd<P, 2>(stress, ncells, nrhs, ndofs, cell_dofs, u, cellJ, coeff, pi_1, op, out, sx, tx, stream);
  default:
    return launch_pd<P, 3>(stress, ncells, nrhs, ndofs, cell_dofs, u, cellJ, coeff, pi_1, op, out, sx, tx, stream);
  }
}

// all pointers but op DEVICE; enqueues on stream
static hipError_t launch_primal_flux(int p, int d, bool stress, int32_t ncells, int32_t nrhs, int64_t ndofs,
                                     const int32_t* cell_dofs, const double* u, const double* cellJ,
                                     const double* coeff, double pi_1, const double* op, double* out,
                                     const StressMuArgs* sx, const FluxTensorArgs* tx, hipStream_t stream)
{
  switch (p)
  {
  case 1:
    return launch_p<1>(d, stress, ncells, nrhs, ndofs, cell_dofs, u, cellJ, coeff, pi_1, op, out, sx, tx, stream);
  case 2:
    return launch_p<2>(d, stress, ncells, nrhs, ndofs, cell_dofs, u, cellJ, coeff, pi_1, op, out, sx, tx, stream);
  case 3:
    return launch_p<3>(d, stress, ncells, nrhs, ndofs, cell_dofs, u, cellJ, coeff, pi_1, op, out, sx, tx, stream);
  default:
    return launch_p<4>(d, stress, ncells, nrhs, ndofs, cell_dofs, u, cellJ, coeff, pi_1, op, out, sx, tx, stream);
  }
}

template <int P>
static int table_p(int d, double* out)
{
  switch (d)
  {
  case 0:
    builtin_table<P, 0>(out);
    break;
  case 1:
    builtin_table<P, 1>(out);
    break;
  case 2:
    builtin_table<P, 2>(out);
    break;
  default:
    builtin_table<P, 3>(out);
  }
  return 2 * nd_of(d) * nd_of(P);
}

// the common body of the entry points; stress: u [ndofs][2], two output rows, coeff = cell_pi1.  shear: the mu / cell_mu
// of eqlb_primal_stress_dg_mu (cell_mu in `memspace`) or nullptr; mu == 1 without an array is the call without it.
// cell_D: the tensor [ncells][3] of eqlb_primal_flux_dg_tensor in `memspace` (flux only) or nullptr
static int primal_flux_call(const char* who, eqlb_mesh_t* mesh, int32_t p, int32_t d, int32_t nrhs, bool stress,
                            const int32_t* cell_dofs, int64_t ndofs, const double* u, const double* coeff,
                            double pi_1, const double* op, double* flux_dg, int32_t memspace, void* stream_,
                            const StressMuArgs* shear = nullptr, const double* cell_D = nullptr)
{
  if (p < 1 || p > PF_PMAX || d < 0 || d > PF_DMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: degrees p = %d, degree_dg = %d outside 1 ... 4, 0 ... 3", who, (int)p,
                (int)d);
  if (nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nrhs = %d", who, (int)nrhs);
  if (!mesh || !cell_dofs || !u || !flux_dg || ndofs < 1 || ndofs > INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: invalid argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  if (shear && !shear->cell_mu)
  {
    EQLB_TRY(check_scalar(who, "mu", *CELL_MU.rule, shear->mu));
    if (shear->mu == 1.0)
      shear = nullptr; // the kernel without the term
  }
  const DeviceMesh& m = mesh->m;
  const int np = nd_of(p), nd = nd_of(d);
  const int32_t ncells = m.ncells;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (memspace == EQLB_MEM_DEVICE)
  {
    const FluxTensorArgs tx{cell_D};
    const hipError_t e = launch_primal_flux(p, d, stress, ncells, nrhs, ndofs, cell_dofs, u, m.cellJ, coeff, pi_1, op,
                                            flux_dg, shear, cell_D ? &tx : nullptr, stream);
    return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
  }
  EQLB_TRY(check_cells(who, ncells, {{CELL_MU, shear ? shear->cell_mu : nullptr}}));
  EQLB_TRY(check_cells(who, ncells, {{CELL_D, cell_D}}));
  // host memory: bad tables are caught here, before anything is launched
  const size_t nidx = (size_t)ncells * np;
  for (size_t i = 0; i < nidx; ++i)
    if (cell_dofs[i] < 0 || (int64_t)cell_dofs[i] >= ndofs)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: cell_dofs[%lld][%d] = %d outside [0, %lld)", who,
                  (long long)(i / np), (int)(i % np), (int)cell_dofs[i], (long long)ndofs);
  const size_t nu = (size_t)ndofs * (stress ? 2 : nrhs), nout = (size_t)(stress ? 2 : nrhs) * ncells * nd * 2;
  HostCall s;
  const auto d_idx = s.in(cell_dofs, nidx);
  const auto d_u = s.in(u, nu), d_c = s.in(coeff, (size_t)ncells);
  const auto d_mu = s.in(shear ? shear->cell_mu : nullptr, (size_t)ncells);
  const auto d_D = s.in(cell_D, 3 * (size_t)ncells);
  const auto d_out = s.out(flux_dg, nout);
  if (s.upload(stream) != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "%s: device allocation failed", who);
  const StressMuArgs sx{shear && shear->cell_mu ? d_mu.get() : nullptr, shear ? shear->mu : 1.0};
  const FluxTensorArgs tx{cell_D ? d_D.get() : nullptr};
  s.note(launch_primal_flux(p, d, stress, ncells, nrhs, ndofs, d_idx, d_u, m.cellJ, d_c, pi_1, op, d_out,
                            shear ? &sx : nullptr, cell_D ? &tx : nullptr, stream));
  const hipError_t e = s.finish(stream);
  return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
}

// ---- eqlb_primal_value_dg ---------------------------------------------------------------------------------------------
template <int P, int D>
static int value_table_pd(double* out)
{
  using T = eqlb_tables::Value<P, D>;
  static_assert(T::NP == nd_of(P) && T::ND == nd_of(D), "table shape");
  for (int i = 0; i < T::ND * T::NP; ++i)
    out[i] = T::PV[i];
  return T::ND * T::NP;
}

template <int P, int D>
static hipError_t launch_value_pd(int32_t ncells, int32_t nrhs, int64_t ndofs, const int32_t* cell_dofs, const double* u,
                                  const double* coeff, const double* op, double* out, hipStream_t stream)
{
  ValueOp<P, D> tab;
  if (op)
    std::memcpy(tab.v, op, sizeof(tab.v));
  else
    value_table_pd<P, D>(tab.v);
  const unsigned grid = (unsigned)(((int64_t)ncells + PF_THREADS - 1) / PF_THREADS);
  hipLaunchKernelGGL((k_primal_value<P, D>), dim3(grid), dim3(PF_THREADS), 0, stream, ncells, nrhs, ndofs, cell_dofs, u,
                     coeff, tab, out);
  return hipGetLastError();
}

// f<P, D>(args...) for the runtime degrees p in 1 ... 4, d in 0 ... 3
#define EQLB_VALUE_DISPATCH(F, p, d, ...)                                                                              \
  [&] {                                                                                                                \
    switch ((p)*4 + (d))                                                                                               \
    {                                                                                                                  \
    case 4: return F<1, 0>(__VA_ARGS__);                                                                               \
    case 5: return F<1, 1>(__VA_ARGS__);                                                                               \
    case 6: return F<1, 2>(__VA_ARGS__);                                                                               \
    case 7: return F<1, 3>(__VA_ARGS__);                                                                               \
    case 8: return F<2, 0>(__VA_ARGS__);                                                                               \
    case 9: return F<2, 1>(__VA_ARGS__);                                                                               \
    case 10: return F<2, 2>(__VA_ARGS__);                                                                              \
    case 11: return F<2, 3>(__VA_ARGS__);                                                                              \
    case 12: return F<3, 0>(__VA_ARGS__);                                                                              \
    case 13: return F<3, 1>(__VA_ARGS__);                                                                              \
    case 14: return F<3, 2>(__VA_ARGS__);                                                                              \
    case 15: return F<3, 3>(__VA_ARGS__);                                                                              \
    case 16: return F<4, 0>(__VA_ARGS__);                                                                              \
    case 17: return F<4, 1>(__VA_ARGS__);                                                                              \
    case 18: return F<4, 2>(__VA_ARGS__);                                                                              \
    default: return F<4, 3>(__VA_ARGS__);                                                                              \
    }                                                                                                                  \
  }()

// all pointers but op DEVICE; enqueues on stream
static hipError_t launch_primal_value(int p, int d, int32_t ncells, int32_t nrhs, int64_t ndofs, const int32_t* cell_dofs,
                                      const double* u, const double* coeff, const double* op, double* out,
                                      hipStream_t stream)
{
  return EQLB_VALUE_DISPATCH(launch_value_pd, p, d, ncells, nrhs, ndofs, cell_dofs, u, coeff, op, out, stream);
}

static int primal_value_call(const char* who, eqlb_mesh_t* mesh, int32_t p, int32_t d, int32_t nrhs,
                             const int32_t* cell_dofs, int64_t ndofs, const double* u, const double* coeff,
                             const double* op, double* value_dg, int32_t memspace, void* stream_)
{
  if (p < 1 || p > PF_PMAX || d < 0 || d > PF_DMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: degrees p = %d, degree_dg = %d outside 1 ... 4, 0 ... 3", who, (int)p,
                (int)d);
  if (nrhs < 1)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: nrhs = %d", who, (int)nrhs);
  if (!mesh || !cell_dofs || !u || !value_dg || ndofs < 1 || ndofs > INT32_MAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: invalid argument", who);
  EQLB_TRY(check_memspace(who, memspace));
  const int np = nd_of(p), nd = nd_of(d);
  const int32_t ncells = mesh->m.ncells;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (memspace == EQLB_MEM_DEVICE)
  {
    const hipError_t e = launch_primal_value(p, d, ncells, nrhs, ndofs, cell_dofs, u, coeff, op, value_dg, stream);
    return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
  }
  // host memory: bad tables are caught here, before anything is launched
  const size_t nidx = (size_t)ncells * np;
  for (size_t i = 0; i < nidx; ++i)
    if (cell_dofs[i] < 0 || (int64_t)cell_dofs[i] >= ndofs)
      return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: cell_dofs[%lld][%d] = %d outside [0, %lld)", who,
                  (long long)(i / np), (int)(i % np), (int)cell_dofs[i], (long long)ndofs);
  HostCall s;
  const auto d_idx = s.in(cell_dofs, nidx);
  const auto d_u = s.in(u, (size_t)ndofs * nrhs), d_c = s.in(coeff, (size_t)ncells);
  const auto d_out = s.out(value_dg, (size_t)nrhs * ncells * nd);
  if (s.upload(stream) != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "%s: device allocation failed", who);
  s.note(launch_primal_value(p, d, ncells, nrhs, ndofs, d_idx, d_u, d_c, op, d_out, stream));
  const hipError_t e = s.finish(stream);
  return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
}

} // namespace eqlb

extern "C" {

int eqlb_primal_value_dg(eqlb_mesh_t* mesh, int32_t p, int32_t degree_dg, int32_t nrhs, const int32_t* cell_dofs,
                         int64_t ndofs, const double* u, const double* cell_coeff, const double* op, double* value_dg,
                         int32_t memspace, void* stream)
{
  return eqlb::primal_value_call("eqlb_primal_value_dg", mesh, p, degree_dg, nrhs, cell_dofs, ndofs, u, cell_coeff, op,
                                 value_dg, memspace, stream);
}

int eqlb_get_value_table(int32_t p, int32_t degree_dg, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (!out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_value_table: null output");
  if (p < 1 || p > PF_PMAX || degree_dg < 0 || degree_dg > PF_DMAX)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_value_table: degrees p = %d, degree_dg = %d outside 1 ... 4, 0 ... 3",
                (int)p, (int)degree_dg);
  if (capacity < nd_of(degree_dg) * nd_of(p))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_value_table: capacity too small");
  return EQLB_VALUE_DISPATCH(value_table_pd, p, degree_dg, out);
}

int eqlb_primal_flux_dg(eqlb_mesh_t* mesh, int32_t p, int32_t degree_dg, int32_t nrhs, const int32_t* cell_dofs,
                        int64_t ndofs, const double* u, const double* cell_coeff, const double* op, double* flux_dg,
                        int32_t memspace, void* stream)
{
  return eqlb::primal_flux_call("eqlb_primal_flux_dg", mesh, p, degree_dg, nrhs, false, cell_dofs, ndofs, u,
                                cell_coeff, 1.0, op, flux_dg, memspace, stream);
}

int eqlb_primal_flux_dg_tensor(eqlb_mesh_t* mesh, int32_t p, int32_t degree_dg, int32_t nrhs, const int32_t* cell_dofs,
                               int64_t ndofs, const double* u, const double* cell_coeff, const double* cell_D,
                               const double* op, double* flux_dg, int32_t memspace, void* stream)
{
  if (!cell_D)
    return fail(EQLB_ERR_INVALID_ARGUMENT,
                "eqlb_primal_flux_dg_tensor: cell_D is null (eqlb_primal_flux_dg is the entry without a tensor)");
  return eqlb::primal_flux_call("eqlb_primal_flux_dg_tensor", mesh, p, degree_dg, nrhs, false, cell_dofs, ndofs, u,
                                cell_coeff, 1.0, op, flux_dg, memspace, stream, nullptr, cell_D);
}

int eqlb_primal_stress_dg(eqlb_mesh_t* mesh, int32_t p, int32_t degree_dg, const int32_t* cell_dofs, int64_t ndofs,
                          const double* u, double pi_1, const double* cell_pi1, const double* op, double* flux_dg,
                          int32_t memspace, void* stream)
{
  return eqlb::primal_flux_call("eqlb_primal_stress_dg", mesh, p, degree_dg, 1, true, cell_dofs, ndofs, u, cell_pi1,
                                pi_1, op, flux_dg, memspace, stream);
}

int eqlb_primal_stress_dg_mu(eqlb_mesh_t* mesh, int32_t p, int32_t degree_dg, const int32_t* cell_dofs, int64_t ndofs,
                             const double* u, double pi_1, const double* cell_pi1, double mu, const double* cell_mu,
                             const double* op, double* flux_dg, int32_t memspace, void* stream)
{
  const eqlb::StressMuArgs shear{cell_mu, mu};
  return eqlb::primal_flux_call("eqlb_primal_stress_dg_mu", mesh, p, degree_dg, 1, true, cell_dofs, ndofs, u, cell_pi1,
                                pi_1, op, flux_dg, memspace, stream, &shear);
}

int eqlb_get_primal_table(int32_t p, int32_t degree_dg, double* out, int32_t capacity)
{
  using namespace eqlb;
  if (p < 1 || p > PF_PMAX || degree_dg < 0 || degree_dg > PF_DMAX || !out)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_primal_table: degrees p = %d, degree_dg = %d outside 1 ... 4, 0 ... 3",
                (int)p, (int)degree_dg);
  if (capacity < 2 * nd_of(degree_dg) * nd_of(p))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_get_primal_table: capacity too small");
  switch (p)
  {
  case 1:
    return table_p<1>(degree_dg, out);
  case 2:
    return table_p<2>(degree_dg, out);
  case 3:
    return table_p<3>(degree_dg, out);
  default:
    return table_p<4>(degree_dg, out);
  }
}

} // extern "C"
