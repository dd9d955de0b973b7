// RT_4 estimator and acceptance kernels for projected data in DG_2, DG_1, DG_0 (see eqlb_estimate_lowdeg.hip).  Their
// reference tensors are not in git: the build writes them (tools/gen_tables.py --build, csrc/Makefile).
#include "eqlb_estimate_kernels.h"
#include "eqlb_tables_build_gen.h"

namespace eqlb
{

int launch_estimate_k4_lowdeg(const DeviceMesh& m, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                              const double* rhs_dg, double* div2, double* sig2, double* jump, double alpha,
                              double beta, hipStream_t stream, const EstWeightArgs* wx)
{
  if (deg == 2)
    return launch_estimate_kd<4, 2>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (deg == 1)
    return launch_estimate_kd<4, 1>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  if (deg == 0)
    return launch_estimate_kd<4, 0>(m, nrhs, x_eq, flux_dg, rhs_dg, div2, sig2, jump, alpha, beta, stream, wx);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_boundary_residual_k4_lowdeg(const DeviceMesh& m, int deg, int nrhs, const double* x_eq,
                                       const double* flux_dg, int32_t nlist, const int32_t* facets,
                                       const double* bvals, double* out, hipStream_t stream)
{
  if (deg == 2)
    return launch_boundary_residual_kd<4, 2>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (deg == 1)
    return launch_boundary_residual_kd<4, 1>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  if (deg == 0)
    return launch_boundary_residual_kd<4, 0>(m, nrhs, x_eq, flux_dg, nlist, facets, bvals, out, stream);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_oscillation_k4_lowdeg(const DeviceMesh& m, int deg, int nrhs, const double* x_eq, const double* flux_dg,
                                 int nq, const double* qpoints, const double* qweights, const double* fvalues,
                                 const double* korn, double* out, hipStream_t stream)
{
  if (deg == 2)
    return launch_oscillation_kd<4, 2>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  if (deg == 1)
    return launch_oscillation_kd<4, 1>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  if (deg == 0)
    return launch_oscillation_kd<4, 0>(m, nrhs, x_eq, flux_dg, nq, qpoints, qweights, fvalues, korn, out, stream);
  return EQLB_ERR_UNSUPPORTED;
}

} // namespace eqlb
