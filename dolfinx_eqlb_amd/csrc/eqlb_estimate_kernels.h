// Acceptance predicates and estimator quantities on the device - the step right after the
// equilibration in the reference's workflows: the divergence / jump checks of
// python/dolfinx_eqlb/eqlb/check_eqlb_conditions.py:183-359 and the cell-wise flux indicator
// of demo/poisson/demo_error_estimation.py:52-124: || sigma_eq ||^2_T for the discontinuous SE flux
// (alpha = 0, beta = 1: the total flux is sigma_eq + G), || sigma_eq - G ||^2_T for a conforming (EV)
// flux given in the broken layout (alpha = -1, beta = 0: the total flux is sigma_eq itself).  Quadrature-free like the patch kernel: with rho = detJ * (Pi f - div(sigma_eq + G)) in
// P_{k-1}(ref) and m_q = int rho mono_q,
//   || Pi f - div(sigma_eq + G) ||^2_T = m^T GMI m / |detJ|,   || sigma_eq ||^2_T = c^T (sum_x g_x S_x) c,
// and the normal-flux jump of sigma_eq + G on an interior facet from the outward moments of both
// cells (reversal matrix B when their facet parameters run against each other).
//
// The data G, f come in DG_d, 0 <= d <= k - 1 (the reference accepts any such degree, se/reconstruction.hpp:363-373):
// every kernel below is a template of (K, DEG) that contracts them with the tensors HG, DM, F0, MRD, MPS of the pair,
// so nothing is embedded into DG_{k-1}.  The DEG = k - 1 instances live in eqlb_estimate.hip, the ones for
// d < k - 1 in eqlb_estimate_lowdeg.hip / eqlb_estimate_lowdeg_k4.hip.
#pragma once

#include "eqlb_device_common.h"
#include "eqlb_host_util.h"
#include <cmath>
#include <vector>
#include "eqlb_tables_gen.h"

namespace eqlb
{

template <int K, int DEG = K - 1>
struct EstTables
{
  using R = eqlb_tables::Ref<K, DEG>;
  static constexpr int NRT = R::NRT, ND = R::ND, NQ = R::NQ;
  static constexpr int OFF_S = 0, OFF_HG = OFF_S + R::S_SIZE, OFF_DM = OFF_HG + R::HG_SIZE,
                       OFF_GMI = OFF_DM + R::DM_SIZE, OFF_F0 = OFF_GMI + R::GMI_SIZE,
                       OFF_MRD = OFF_F0 + R::F0_SIZE, OFF_MPS = OFF_MRD + R::MRD_SIZE,
                       TOTAL = OFF_MPS + R::MPS_SIZE;
  static void fill(std::vector<double>& t)
  {
    t.clear();
    t.insert(t.end(), R::S, R::S + R::S_SIZE);
    t.insert(t.end(), R::HG, R::HG + R::HG_SIZE);
    t.insert(t.end(), R::DM, R::DM + R::DM_SIZE);
    t.insert(t.end(), R::GMI, R::GMI + R::GMI_SIZE);
    t.insert(t.end(), R::F0, R::F0 + R::F0_SIZE);
    t.insert(t.end(), R::MRD, R::MRD + R::MRD_SIZE);
    t.insert(t.end(), R::MPS, R::MPS + R::MPS_SIZE);
  }
};

// k_estimate_cells<K, DEG> and, from the same source (eqlb_estimate_cells.inc), k_estimate_cells_weighted<K, DEG>: the
// flux norm in the energy norm of -div(kappa D grad u), cell_sig2 = int_T (sigma_eq - sigma_h)^T W (sigma_eq - sigma_h)
// with W = adj(D) / (kappa det D) formed per cell from `wx` (eqlb_se_estimate_weighted / eqlb_ev_estimate_weighted).  A
// kernel of its own, so that the entries without a weight launch the symbols, arguments and code they launched before
// (tools/isa_compare.py); it forms cell_sig2 only - the divergence residual of a weighted call comes from
// k_estimate_cells itself and is therefore bit for bit the one of the unweighted entry.
#define EQLB_EST_WEIGHTED 0
#include "eqlb_estimate_cells.inc"
#undef EQLB_EST_WEIGHTED
#define EQLB_EST_WEIGHTED 1
#include "eqlb_estimate_cells.inc"
#undef EQLB_EST_WEIGHTED

// outward moments of (sigma_eq + G) on local facet lf of cell c
template <int K, int DEG>
__device__ __forceinline__ void facet_moments(const double* st, const double* cellJ, const double* x_eq,
                                              const double* flux_dg, int32_t c, int lf, double beta,
                                              double* mu)
{
  using E = EstTables<K, DEG>;
  constexpr int NRT = E::NRT, ND = E::ND;
  const double* J = cellJ + 4 * (int64_t)c;
  const double detJ = J[0] * J[3] - J[1] * J[2];
  const double sgn = (detJ > 0.0) ? 1.0 : -1.0, pf = (lf == 1) ? sgn : -sgn;
  const double a00 = J[3], a01 = -J[1], a10 = -J[2], a11 = J[0];
  const double nx = (lf == 2) ? 0.0 : -1.0, ny = (lf == 0) ? -1.0 : ((lf == 1) ? 0.0 : 1.0);
  const double nu0 = a00 * nx + a10 * ny, nu1 = a01 * nx + a11 * ny; // adj^T N_f
#pragma unroll
  for (int j = 0; j < K; ++j)
    mu[j] = x_eq[(int64_t)c * NRT + lf * K + j];
  const double* G = flux_dg + (int64_t)c * ND * 2;
#pragma unroll
  for (int i = 0; i < ND; ++i)
  {
    const double gn = beta * (G[2 * i] * nu0 + G[2 * i + 1] * nu1);
#pragma unroll
    for (int j = 0; j < K; ++j)
      mu[j] += st[E::OFF_F0 + (lf * ND + i) * K + j] * gn;
  }
#pragma unroll
  for (int j = 0; j < K; ++j)
    mu[j] *= pf;
}

// one thread per facet: max_j |moment_j of the normal-flux jump| (0 on boundary facets)
template <int K, int DEG>
__global__ void __launch_bounds__(256)
k_estimate_facets(int32_t nfacets, const double* __restrict__ tab, const double* __restrict__ cellJ,
                  const int32_t* __restrict__ cell_facets, const uint8_t* __restrict__ facet_perm,
                  const int32_t* __restrict__ facet_cells_off, const int32_t* __restrict__ facet_cells,
                  const double* __restrict__ x_eq, const double* __restrict__ flux_dg,
                  double* __restrict__ jump, const double beta)
{
  using E = EstTables<K, DEG>;
  extern __shared__ double st[];
  for (int i = threadIdx.x; i < E::TOTAL; i += 256)
    st[i] = tab[i];
  __syncthreads();
  const int32_t fct = blockIdx.x * 256 + threadIdx.x;
  if (fct >= nfacets)
    return;
  const int32_t o = facet_cells_off[fct];
  if (facet_cells_off[fct + 1] - o < 2)
  {
    jump[fct] = 0.0;
    return;
  }
  const int32_t c0 = facet_cells[o], c1 = facet_cells[o + 1];
  int l0 = 0, l1 = 0;
#pragma unroll
  for (int l = 1; l < 3; ++l)
  {
    if (cell_facets[(int64_t)c0 * 3 + l] == fct)
      l0 = l;
    if (cell_facets[(int64_t)c1 * 3 + l] == fct)
      l1 = l;
  }
  double m0[K], m1[K];
  facet_moments<K, DEG>(st, cellJ, x_eq, flux_dg, c0, l0, beta, m0);
  facet_moments<K, DEG>(st, cellJ, x_eq, flux_dg, c1, l1, beta, m1);
  const bool rev = facet_perm[(int64_t)c0 * 3 + l0] != facet_perm[(int64_t)c1 * 3 + l1];
  double worst = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j)
  {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i)
      t += (rev ? bcoef(j, i) : ((i == j) ? 1.0 : 0.0)) * m1[i];
    worst = fmax(worst, fabs(m0[j] + t));
  }
  jump[fct] = worst;
}

// Flux boundary condition (check_boundary_conditions, python/dolfinx_eqlb/eqlb/check_eqlb_conditions.py:90-179):
// one thread per listed boundary facet, out = max_j | facet DOF j of (sigma_eq + G) - boundary DOF j |, seen from
// the facet's first cell.  In the hierarchic basis the facet DOFs are the moments of the (reference) normal flux
// against s^j, those of G come from F0 of the pair.  flux_dg == nullptr: a conforming flux, sigma_eq is the total
// flux; bvals == nullptr: homogeneous condition.  A facet id outside the mesh gives NaN and reads nothing.
template <int K, int DEG>
__global__ void __launch_bounds__(256)
k_boundary_residual(int32_t nlist, int32_t nfacets, const int32_t* __restrict__ facets,
                    const double* __restrict__ f0, const double* __restrict__ cellJ,
                    const int32_t* __restrict__ cell_facets, const int32_t* __restrict__ facet_cells_off,
                    const int32_t* __restrict__ facet_cells, const double* __restrict__ x_eq,
                    const double* __restrict__ flux_dg, const double* __restrict__ bvals, double* __restrict__ out)
{
  using R = eqlb_tables::Ref<K, DEG>;
  constexpr int NRT = R::NRT, ND = R::ND;
  const int32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nlist)
    return;
  const int32_t fct = facets[t];
  if (fct < 0 || fct >= nfacets)
  {
    out[t] = __builtin_nan("");
    return;
  }
  const int32_t c = facet_cells[facet_cells_off[fct]];
  int lf = 0;
#pragma unroll
  for (int l = 1; l < 3; ++l)
    if (cell_facets[(int64_t)c * 3 + l] == fct)
      lf = l;
  const double* dofs = x_eq + (int64_t)c * NRT + lf * K;
  double mu[K];
#pragma unroll
  for (int j = 0; j < K; ++j)
    mu[j] = dofs[j];
  if (flux_dg)
  {
    const double* J = cellJ + 4 * (int64_t)c;
    const double a00 = J[3], a01 = -J[1], a10 = -J[2], a11 = J[0];
    const double nx = (lf == 2) ? 0.0 : -1.0, ny = (lf == 0) ? -1.0 : ((lf == 1) ? 0.0 : 1.0);
    const double nu0 = a00 * nx + a10 * ny, nu1 = a01 * nx + a11 * ny; // adj^T N_f
    const double* G = flux_dg + (int64_t)c * ND * 2;
#pragma unroll
    for (int i = 0; i < ND; ++i)
    {
      const double gn = G[2 * i] * nu0 + G[2 * i + 1] * nu1;
#pragma unroll
      for (int j = 0; j < K; ++j)
        mu[j] += f0[(lf * ND + i) * K + j] * gn;
    }
  }
  double worst = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j)
    worst = fmax(worst, fabs(bvals ? mu[j] - bvals[(int64_t)c * NRT + lf * K + j] : mu[j]));
  out[t] = worst;
}

template <int K, int DEG>
static int launch_estimate_kd(const DeviceMesh& m, int nrhs, const double* x_eq, const double* flux_dg,
                              const double* rhs_dg, double* div2, double* sig2, double* jump, double alpha,
                              double beta, hipStream_t stream, const EstWeightArgs* wx = nullptr)
{
  using E = EstTables<K, DEG>;
  std::vector<double> t;
  E::fill(t);
  DevBuf<double> d_t;
  if (d_t.alloc(t.size()))
    return EQLB_ERR_DEVICE;
  hipError_t e = hipMemcpyAsync(d_t, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, stream);
  const size_t lds = t.size() * sizeof(double);
  const int64_t nx = (int64_t)m.ncells * E::NRT, ng = (int64_t)m.ncells * E::ND * 2, nf = (int64_t)m.ncells * E::ND;
  for (int r = 0; r < nrhs && e == hipSuccess; ++r)
  {
    if (wx && sig2) // the weighted flux norm by its own kernel; the divergence residual by the one below, as it was
    {
      if (div2)
        hipLaunchKernelGGL((k_estimate_cells<K, DEG>), dim3((m.ncells + 255) / 256), dim3(256), lds, stream, m.ncells,
                           d_t, m.cellJ, x_eq + r * nx, flux_dg + r * ng, rhs_dg + r * nf,
                           div2 + (int64_t)r * m.ncells, static_cast<double*>(nullptr), alpha, beta);
      hipLaunchKernelGGL((k_estimate_cells_weighted<K, DEG>), dim3((m.ncells + 255) / 256), dim3(256), lds, stream,
                         m.ncells, d_t, m.cellJ, x_eq + r * nx, flux_dg + r * ng, sig2 + (int64_t)r * m.ncells, alpha,
                         *wx);
    }
    else if (div2 || sig2)
      hipLaunchKernelGGL((k_estimate_cells<K, DEG>), dim3((m.ncells + 255) / 256), dim3(256), lds, stream, m.ncells,
                         d_t, m.cellJ, x_eq + r * nx, flux_dg + r * ng, rhs_dg + r * nf,
                         div2 ? div2 + (int64_t)r * m.ncells : nullptr,
                         sig2 ? sig2 + (int64_t)r * m.ncells : nullptr, alpha, beta);
    if (jump)
      hipLaunchKernelGGL((k_estimate_facets<K, DEG>), dim3((m.nfacets + 255) / 256), dim3(256), lds, stream,
                         m.nfacets, d_t, m.cellJ, m.cell_facets, m.facet_perm, m.facet_cells_off,
                         m.facet_cells, x_eq + r * nx, flux_dg + r * ng, jump + (int64_t)r * m.nfacets, beta);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipStreamSynchronize(stream); // the table buffer ends with this call
  return (e == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

// [nrhs][nlist] residuals of the flux boundary condition on the listed facets (DEVICE pointers)
template <int K, int DEG>
static int launch_boundary_residual_kd(const DeviceMesh& m, int nrhs, const double* x_eq, const double* flux_dg,
                                       int32_t nlist, const int32_t* facets, const double* bvals, double* out,
                                       hipStream_t stream)
{
  using R = eqlb_tables::Ref<K, DEG>;
  DevBuf<double> d_t;
  if (d_t.alloc(R::F0_SIZE))
    return EQLB_ERR_DEVICE;
  hipError_t e = hipMemcpyAsync(d_t, R::F0, R::F0_SIZE * sizeof(double), hipMemcpyHostToDevice, stream);
  const int64_t nx = (int64_t)m.ncells * R::NRT, ng = (int64_t)m.ncells * R::ND * 2;
  for (int r = 0; r < nrhs && e == hipSuccess; ++r)
  {
    hipLaunchKernelGGL((k_boundary_residual<K, DEG>), dim3((nlist + 255) / 256), dim3(256), 0, stream, nlist,
                       m.nfacets, facets, d_t, m.cellJ, m.cell_facets, m.facet_cells_off, m.facet_cells,
                       x_eq + r * nx, flux_dg ? flux_dg + r * ng : nullptr, bvals ? bvals + r * nx : nullptr,
                       out + (int64_t)r * nlist);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipStreamSynchronize(stream); // the table buffer ends with this call
  return (e == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

// ---- data oscillation ((h_T / pi) || f - div sigma ||_T of demo/poisson/demo_error_estimation.py:93-100,
//      with the Korn constant in front for stresses, demo/elasticity/demo_error_estimation.py:104-106) -------
// detJ * div(sigma_eq + beta G) is a polynomial of P_{k-1}(ref): its monomial coefficients are GMI * (moments),
// the moments as in k_estimate_cells.  f comes as point values at the images of a reference rule.
// qtab: [nq][NQ] monomial values at the points, then [nq] weights.
template <int K, int DEG>
__global__ void __launch_bounds__(256)
k_oscillation_cells(int32_t ncells, const double* __restrict__ tab, const double* __restrict__ qtab, int nq,
                    const double* __restrict__ cellJ, const double* __restrict__ x_eq,
                    const double* __restrict__ flux_dg, const double* __restrict__ fvalues,
                    const double* __restrict__ korn, double* __restrict__ out)
{
  using E = EstTables<K, DEG>;
  constexpr int NRT = E::NRT, ND = E::ND, NQ = E::NQ;
  extern __shared__ double st[];
  double* sq = st + E::TOTAL;
  for (int i = threadIdx.x; i < E::TOTAL; i += 256)
    st[i] = tab[i];
  for (int i = threadIdx.x; i < nq * (NQ + 1); i += 256)
    sq[i] = qtab[i];
  __syncthreads();
  const int32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells)
    return;
  const double* J = cellJ + 4 * (int64_t)c;
  const double J00 = J[0], J01 = J[1], J10 = J[2], J11 = J[3];
  const double detJ = J00 * J11 - J01 * J10;
  const double a00 = J11, a01 = -J01, a10 = -J10, a11 = J00;
  const double* cf = x_eq + (int64_t)c * NRT;
  double m[NQ];
  m[0] = -cf[0] + cf[K] - cf[2 * K];
#pragma unroll
  for (int q = 1; q < NQ; ++q)
    m[q] = cf[3 * K + q - 1];
  if (flux_dg && !(DEG == 0 && K >= 2)) // P0 data: div G = 0 (RT_1 keeps the generic contraction)
  {
    const double* G = flux_dg + (int64_t)c * ND * 2;
#pragma unroll
    for (int i = 0; i < ND; ++i)
    {
      const double gx = G[2 * i], gy = G[2 * i + 1];
      const double h0 = a00 * gx + a01 * gy, h1 = a10 * gx + a11 * gy;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        m[q] += h0 * st[E::OFF_DM + (i * 2 + 0) * NQ + q] + h1 * st[E::OFF_DM + (i * 2 + 1) * NQ + q];
    }
  }
  double a[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    double r = 0.0;
#pragma unroll
    for (int p = 0; p < NQ; ++p)
      r += st[E::OFF_GMI + q * NQ + p] * m[p];
    a[q] = r / detJ;
  }
  const double* fv = fvalues + (int64_t)c * nq;
  double s = 0.0;
  for (int q = 0; q < nq; ++q)
  {
    double d = fv[q];
#pragma unroll
    for (int p = 0; p < NQ; ++p)
      d -= a[p] * sq[q * NQ + p];
    s += sq[nq * NQ + q] * d * d;
  }
  // cell diameter as dolfinx::mesh::h: the longest edge of the triangle
  const double e1 = J00 * J00 + J10 * J10, e2 = J01 * J01 + J11 * J11,
               e3 = (J01 - J00) * (J01 - J00) + (J11 - J10) * (J11 - J10);
  const double h2 = fmax(e1, fmax(e2, e3));
  const double ck = korn ? korn[c] : 1.0;
  constexpr double PI = 3.14159265358979323846;
  out[c] = ck * ck * h2 / (PI * PI) * fabs(detJ) * s;
}

template <int K, int DEG>
static int launch_oscillation_kd(const DeviceMesh& m, int nrhs, const double* x_eq, const double* flux_dg, int nq,
                                 const double* qpoints, const double* qweights, const double* fvalues,
                                 const double* korn, double* out, hipStream_t stream)
{
  using E = EstTables<K, DEG>;
  using R = eqlb_tables::Ref<K, DEG>;
  std::vector<double> t;
  E::fill(t);
  std::vector<double> qt((size_t)nq * (E::NQ + 1));
  for (int q = 0; q < nq; ++q)
  {
    for (int p = 0; p < E::NQ; ++p)
      qt[(size_t)q * E::NQ + p] = std::pow(qpoints[2 * q], R::MONO_X[p]) * std::pow(qpoints[2 * q + 1], R::MONO_Y[p]);
    qt[(size_t)nq * E::NQ + q] = qweights[q];
  }
  DevBuf<double> d_t, d_q;
  if (d_t.alloc(t.size()) || d_q.alloc(qt.size()))
    return EQLB_ERR_DEVICE;
  hipError_t e = hipMemcpyAsync(d_t, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_q, qt.data(), qt.size() * sizeof(double), hipMemcpyHostToDevice, stream);
  const size_t lds = (t.size() + qt.size()) * sizeof(double);
  const int64_t nx = (int64_t)m.ncells * E::NRT, ng = (int64_t)m.ncells * E::ND * 2;
  for (int r = 0; r < nrhs && e == hipSuccess; ++r)
  {
    hipLaunchKernelGGL((k_oscillation_cells<K, DEG>), dim3((m.ncells + 255) / 256), dim3(256), lds, stream, m.ncells, d_t,
                       d_q, nq, m.cellJ, x_eq + r * nx, flux_dg ? flux_dg + r * ng : nullptr,
                       fvalues + (int64_t)r * m.ncells * nq, korn, out + (int64_t)r * m.ncells);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipStreamSynchronize(stream); // the table buffers end with this call
  return (e == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

} // namespace eqlb
