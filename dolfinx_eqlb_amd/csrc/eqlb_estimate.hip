// Acceptance predicates and estimator quantities (eqlb_estimate_kernels.h): the instances at DEG = k - 1, the
// stress estimator, and the dispatchers that hand a lower data degree to eqlb_estimate_lowdeg.hip.
#include "eqlb_estimate_kernels.h"

namespace eqlb
{

int launch_estimate(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                    const double* rhs_dg, double* div2, double* sig2, double* jump, double alpha,
                    double beta, hipStream_t stream, const EstWeightArgs* wx)
{
  if (deg != k - 1)
    return launch_estimate_lowdeg(m, k, deg, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (k == 1)
    return launch_estimate_kd<1, 0>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (k == 2)
    return launch_estimate_kd<2, 1>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (k == 3)
    return launch_estimate_kd<3, 2>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (k == 4)
    return launch_estimate_kd<4, 3>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_boundary_residual(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq,
                             const double* flux_dg, int32_t nlist, const int32_t* facets, const double* bvals,
                             double* out, hipStream_t stream)
{
  if (deg != k - 1)
    return launch_boundary_residual_lowdeg(m, k, deg, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (k == 1)
    return launch_boundary_residual_kd<1, 0>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (k == 2)
    return launch_boundary_residual_kd<2, 1>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (k == 3)
    return launch_boundary_residual_kd<3, 2>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (k == 4)
    return launch_boundary_residual_kd<4, 3>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  return EQLB_ERR_UNSUPPORTED;
}

// ---- stress estimator (demo/elasticity/demo_error_estimation.py:49-148) --------------------------------
// delta_sigma = (row 0; row 1) of an equilibrated stress.  Per cell, with W^{ab}_{rs} = c_r^T SU^{ab} c_s on the
// reference cell and int_T sigma_r^x sigma_s^y = (1/|detJ|) sum_ab J_xa J_yb W^{ab}_{rs}:
//   energy = int delta_sigma : A delta_sigma,  A tau = (tau - pi_1/(2 + 2 pi_1) tr(tau) I) / 2        (:100-102,109)
//   wsym   = int (C_K (dsig_01 - dsig_10) / 2)^2                                                         (:108,121)
//   asym3  = int (dsig_01 - dsig_10) hat_v  per vertex (the weak symmetry condition,
//            python/dolfinx_eqlb/eqlb/check_eqlb_conditions.py:476-521, before assembly over the nodes)
// With a shear modulus (eqlb_se_estimate_stress_mu): sigma = mu_T (2 eps + pi_T div I), A_T = A(pi_T) / mu_T, and the Korn
// bound of the weak-symmetry term picks up 1 / mu_T as well: energy and wsym are divided by mu_T, asym3 is unchanged.
#define EQLB_EST_MU 0
#include "eqlb_estimate_stress_cells.inc"
#undef EQLB_EST_MU
#define EQLB_EST_MU 1
#include "eqlb_estimate_stress_cells.inc"
#undef EQLB_EST_MU

// node value = sum of the vertex values of the cells around the node, in the order of the CSR list
__global__ void __launch_bounds__(256)
k_gather_vertex_values(int32_t nnodes, const int32_t* __restrict__ node_cells_off,
                       const int32_t* __restrict__ node_cells, const int32_t* __restrict__ cell_nodes,
                       const double* __restrict__ val3, double* __restrict__ out)
{
  const int32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= nnodes)
    return;
  double s = 0.0;
  for (int32_t o = node_cells_off[n]; o < node_cells_off[n + 1]; ++o)
  {
    const int32_t c = node_cells[o];
    const int v = (cell_nodes[(int64_t)c * 3 + 1] == n) ? 1 : ((cell_nodes[(int64_t)c * 3 + 2] == n) ? 2 : 0);
    s += val3[(int64_t)c * 3 + v];
  }
  out[n] = s;
}

template <int K>
static int launch_estimate_stress_k(const DeviceMesh& m, const int32_t* node_cells, const double* x0,
                                    const double* x1, const double* korn, double pi_1, const StressCoeffArgs* co,
                                    double* energy, double* wsym, double* node_asym, hipStream_t stream)
{
  using R = eqlb_tables::Ref<K, K - 1>;
  std::vector<double> t(R::SU, R::SU + R::SU_SIZE);
  t.insert(t.end(), R::V, R::V + R::V_SIZE);
  DevBuf<double> d_t, d_a;
  if (d_t.alloc(t.size()) || (node_asym && d_a.alloc(3 * (size_t)m.ncells)))
    return EQLB_ERR_DEVICE;
  hipError_t e = hipMemcpyAsync(d_t, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
  {
    if (co) // the variant with cell-wise coefficients; without them the launch as before they existed
      hipLaunchKernelGGL(k_estimate_stress_cells_mu<K>, dim3((m.ncells + 255) / 256), dim3(256),
                         t.size() * sizeof(double), stream, m.ncells, d_t, m.cellJ, x0, x1, korn, *co, energy, wsym,
                         d_a);
    else
      hipLaunchKernelGGL(k_estimate_stress_cells<K>, dim3((m.ncells + 255) / 256), dim3(256),
                         t.size() * sizeof(double), stream, m.ncells, d_t, m.cellJ, x0, x1, korn, pi_1, energy, wsym,
                         d_a);
    if (node_asym)
      hipLaunchKernelGGL(k_gather_vertex_values, dim3((m.nnodes + 255) / 256), dim3(256), 0, stream, m.nnodes,
                         m.node_cells_off, node_cells, m.cell_nodes, d_a, node_asym);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipStreamSynchronize(stream); // the buffers end with this call
  return (e == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

int launch_estimate_stress(const DeviceMesh& m, const int32_t* node_cells, int k, const double* x0,
                           const double* x1, const double* korn, double pi_1, double* energy, double* wsym,
                           double* node_asym, hipStream_t stream, const StressCoeffArgs* co)
{
  if (k == 1)
    return launch_estimate_stress_k<1>(m, node_cells, x0, x1, korn, pi_1, co, energy, wsym, node_asym, stream);
  if (k == 2)
    return launch_estimate_stress_k<2>(m, node_cells, x0, x1, korn, pi_1, co, energy, wsym, node_asym, stream);
  if (k == 3)
    return launch_estimate_stress_k<3>(m, node_cells, x0, x1, korn, pi_1, co, energy, wsym, node_asym, stream);
  if (k == 4)
    return launch_estimate_stress_k<4>(m, node_cells, x0, x1, korn, pi_1, co, energy, wsym, node_asym, stream);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_oscillation(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                       int nq, const double* qpoints, const double* qweights, const double* fvalues,
                       const double* korn, double* out, hipStream_t stream)
{
  if (deg != k - 1)
    return launch_oscillation_lowdeg(m, k, deg, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out,
                                     stream);
  if (k == 1)
    return launch_oscillation_kd<1, 0>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  if (k == 2)
    return launch_oscillation_kd<2, 1>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  if (k == 3)
    return launch_oscillation_kd<3, 2>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  if (k == 4)
    return launch_oscillation_kd<4, 3>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  return EQLB_ERR_UNSUPPORTED;
}

} // namespace eqlb
