// The exact solve on the coarsest level of a hierarchy (eqlb_hierarchy_set_coarse of include/eqlb.h): what
// eqlb_multilevel.hip sees of eqlb_coarse.hip.  Host code only.
#pragma once

#include "eqlb_host_util.h"

namespace eqlb
{
// The dense factor of level 0 on its free rows, owned by the hierarchy handle: a snapshot of the mask and the
// coefficient of level 0 at the last coarse_setup.  All arrays DEVICE; they grow with n and are kept until the handle
// ends.
struct CoarseSolve
{
  int on = 0;          // the switch: the level-0 combine is replaced by coarse_apply
  int32_t n = 0;       // free rows of level 0
  int64_t n0 = 0;      // rows of level 0
  int32_t cap = -1;    // rows the arrays below hold
  DevBuf<int32_t> rows;   // [n] ascending
  DevBuf<double> d;       // [n] the pivots
  DevBuf<double> W;       // [n][n] row-major, unit lower triangular: L^-1
  DevBuf<double> Wt;      // [n][n] the transpose of W (during the set-up: A_0 and its Schur complements)
  DevBuf<double> panel;   // [n][COARSE_BLOCK] the multipliers l of the current block of columns
  DevBuf<double> y;       // [MANY_R][n] between the two passes of an application
  DevBuf<int32_t> status; // [1] 0, or 1 + the first pivot that was not > 0
};

// Factors level 0 again on `stream` and waits for it; switches cs.on on if that worked and leaves it off otherwise:
// EQLB_ERR_INVALID_ARGUMENT (a component without a Dirichlet DOF), EQLB_ERR_UNSUPPORTED (more than COARSE_MAX_ROWS free
// rows, before anything is allocated), EQLB_ERR_SINGULAR (a pivot that is not > 0)
int coarse_setup(const char* who, CoarseSolve& cs, const SolverLevel& lv, hipStream_t stream);

// z_0 = W^T ((W r_0[rows]) / d) on the free rows and 0 on the fixed ones, on the columns of c; r, z DEVICE [R][n0]: two
// launches (one if there is no free row)
hipError_t coarse_apply(const CoarseSolve& cs, const ManyCols& c, const double* r, const uint8_t* fixed, double* z,
                        hipStream_t stream);
} // namespace eqlb
