// RT_4 patch kernels for projected data in DG_2, DG_1, DG_0 (see eqlb_se_kernels_lowdeg.hip): the per-bin launches of
// launch_k4 - register solver (SE, and EV on the slot path) and dense LDS Cholesky - at DEG < 3.  Their 63 instances
// are the largest part of the lower-degree build; in a translation unit of their own they compile in parallel with
// the rest.  Their reference tensors (0.4 MB of literals) are not in git: the build writes them
// (tools/gen_tables.py --build, csrc/Makefile).
#include "eqlb_se_launch.h"
#include "eqlb_tables_build_gen.h"

namespace eqlb
{

int fill_tables_k4_lowdeg(int deg, std::vector<double>& out)
{
  if (deg == 2)
    fill_tables_t<4, 2>(out);
  else if (deg == 1)
    fill_tables_t<4, 1>(out);
  else if (deg == 0)
    fill_tables_t<4, 0>(out);
  else
    return EQLB_ERR_UNSUPPORTED;
  return 0;
}

int launch_se_patch_k4_lowdeg(int deg, int P, int solver, int scatter, const SeArgs& a, hipStream_t stream, int mode)
{
  if (deg == 2)
    return launch_k4<2>(P, solver, scatter, a, stream, mode);
  if (deg == 1)
    return launch_k4<1>(P, solver, scatter, a, stream, mode);
  if (deg == 0)
    return launch_k4<0>(P, solver, scatter, a, stream, mode);
  return EQLB_ERR_UNSUPPORTED;
}

} // namespace eqlb
