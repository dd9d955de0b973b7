// Estimator and acceptance kernels for projected data of a degree below k - 1 (see eqlb_se_kernels_lowdeg.hip for
// the equilibrators): the instances of the bodies of eqlb_estimate_kernels.h at (K, DEG) = (2, 0), (3, 1), (3, 0); k = 4
// with DEG = 2, 1, 0 in eqlb_estimate_lowdeg_k4.hip.  flux_dg / rhs_dg are read in DG_d with the tensors HG, DM, F0,
// MRD, MPS of the pair - no embedding pass and no temporary of DG_{k-1} size.  A translation unit of its own, so
// that the code objects of the DEG = k - 1 kernels in eqlb_estimate.hip stay as they are.
#include "eqlb_estimate_kernels.h"

namespace eqlb
{

int launch_estimate_lowdeg(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                           const double* rhs_dg, double* div2, double* sig2, double* jump, double alpha,
                           double beta, hipStream_t stream, const EstWeightArgs* wx)
{
  if (k == 4)
    return launch_estimate_k4_lowdeg(m, deg, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (k == 2 && deg == 0)
    return launch_estimate_kd<2, 0>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (k == 3 && deg == 1)
    return launch_estimate_kd<3, 1>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (k == 3 && deg == 0)
    return launch_estimate_kd<3, 0>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_boundary_residual_lowdeg(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq,
                                    const double* flux_dg, int32_t nlist, const int32_t* facets,
                                    const double* bvals, double* out, hipStream_t stream)
{
  if (k == 4)
    return launch_boundary_residual_k4_lowdeg(m, deg, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (k == 2 && deg == 0)
    return launch_boundary_residual_kd<2, 0>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (k == 3 && deg == 1)
    return launch_boundary_residual_kd<3, 1>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (k == 3 && deg == 0)
    return launch_boundary_residual_kd<3, 0>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_oscillation_lowdeg(const DeviceMesh& m, int k, int deg, int nrhs, const double* x_eq,
                              const double* flux_dg, int nq, const double* qpoints, const double* qweights,
                              const double* fvalues, const double* korn, double* out, hipStream_t stream)
{
  if (k == 4)
    return launch_oscillation_k4_lowdeg(m, deg, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out,
                                        stream);
  if (k == 2 && deg == 0)
    return launch_oscillation_kd<2, 0>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  if (k == 3 && deg == 1)
    return launch_oscillation_kd<3, 1>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  if (k == 3 && deg == 0)
    return launch_oscillation_kd<3, 0>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  return EQLB_ERR_UNSUPPORTED;
}

} // namespace eqlb
