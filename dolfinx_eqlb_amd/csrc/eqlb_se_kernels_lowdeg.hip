// Patch kernels for projected data of a degree below k - 1: RT_k with flux_dg / rhs_dg in DG_d, d < k - 1, which the
// reference accepts for any d <= k - 1 (se/reconstruction.hpp:363-373) and its unit tests produce from P_{k-1} primal
// solutions (d = k - 2).  The instances of the templates of eqlb_se_launch.h and eqlb_se_tile.h at (K, DEG) = (2, 0), (3, 1), (3, 0)
// for every launch family that runs at DEG = k - 1: tiled (single and multi right-hand side, SE and EV), fused slot
// launches, per-bin launches; k = 4 with DEG = 2, 1, 0 in eqlb_se_kernels_lowdeg_k4.hip.  The data are read in DG_d
// directly - the tensors F, H, D, HG, WG of the pair (tools/gen_tables.py) - so nothing is embedded into DG_{k-1}.
// Translation units of their own: they compile in parallel with eqlb_se_kernels.hip, whose instances they leave alone.
#include "eqlb_se_launch.h"
#include "eqlb_se_tile.h"

namespace eqlb
{

// LDS of a tiled launch with tiles of tc cells: the tables of a lower data degree are smaller than those of
// DEG = k - 1, so every tile size the tile builder picks for k (tile_cells_of, tile_cells_ev_of, "tile_cells" up to
// tile_cells_max_c) fits
template <int K, int DEG, int MODE>
constexpr size_t tiled_lds_bytes(int tc)
{
  using Z = Sizes<K, DEG, 8>;
  return sizeof(double)
         * ((size_t)(K == 3 ? Z::NTAB_HALF : Z::NTAB) + (MODE ? (size_t)Z::NEV : 0) + (size_t)tc * 3 * (Z::NRT - K));
}
constexpr int TCM2 = tile_cells_max_c(2), TCM3 = tile_cells_max_c(3), TCE3 = EQLB_TILE_CELLS_K3_EV;
static_assert(tiled_lds_bytes<2, 0, 0>(TCM2) <= tiled_lds_bytes<2, 1, 0>(TCM2)
                  && tiled_lds_bytes<2, 0, 1>(TCM2) <= tiled_lds_bytes<2, 1, 1>(TCM2)
                  && tiled_lds_bytes<2, 1, 1>(TCM2) <= 80 * 1024,
              "RT_2 / DG_0 tile: two workgroups per CU");
static_assert(tiled_lds_bytes<3, 0, 0>(TCM3) <= tiled_lds_bytes<3, 1, 0>(TCM3)
                  && tiled_lds_bytes<3, 1, 0>(TCM3) <= tiled_lds_bytes<3, 2, 0>(TCM3)
                  && tiled_lds_bytes<3, 2, 0>(TCM3) <= 160 * 1024,
              "RT_3 / DG_0, DG_1 tile (SE)");
static_assert(tiled_lds_bytes<3, 0, 1>(TCE3) <= tiled_lds_bytes<3, 1, 1>(TCE3)
                  && tiled_lds_bytes<3, 1, 1>(TCE3) <= tiled_lds_bytes<3, 2, 1>(TCE3)
                  && tiled_lds_bytes<3, 2, 1>(TCE3) <= 160 * 1024,
              "RT_3 / DG_0, DG_1 tile (EV)");

int launch_se_patch_tiled_lowdeg(int k, int deg, int mode, const SeArgs& a, const TileArgs& t, hipStream_t stream)
{
  if (k == 2 && deg == 0)
    return mode ? launch_tiled_kd<2, 0, 1>(a, t, stream) : launch_tiled_kd<2, 0, 0>(a, t, stream);
  if (k == 3 && deg == 1)
    return mode ? launch_tiled_kd<3, 1, 1>(a, t, stream) : launch_tiled_kd<3, 1, 0>(a, t, stream);
  if (k == 3 && deg == 0)
    return mode ? launch_tiled_kd<3, 0, 1>(a, t, stream) : launch_tiled_kd<3, 0, 0>(a, t, stream);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_se_patch_tiled_multi_lowdeg(int k, int deg, int mode, const SeArgs& a, const TileArgs& t,
                                       const MultiRhs& mr, hipStream_t stream)
{
  if (k == 2 && deg == 0)
    return mode ? launch_tiled_multi_kd<2, 0, 1>(a, t, mr, stream) : launch_tiled_multi_kd<2, 0, 0>(a, t, mr, stream);
  if (k == 3 && deg == 1)
    return mode ? launch_tiled_multi_kd<3, 1, 1>(a, t, mr, stream) : launch_tiled_multi_kd<3, 1, 0>(a, t, mr, stream);
  if (k == 3 && deg == 0)
    return mode ? launch_tiled_multi_kd<3, 0, 1>(a, t, mr, stream) : launch_tiled_multi_kd<3, 0, 0>(a, t, mr, stream);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_se_patch_fused_lowdeg(int k, int deg, int scatter, const SeArgs& a, const FusedBins& fb,
                                 hipStream_t stream)
{
  if (k == 2 && deg == 0)
    return launch_fused_kd<2, 0>(scatter, a, fb, stream);
  if (k == 3 && deg == 1)
    return launch_fused_kd<3, 1>(scatter, a, fb, stream);
  if (k == 3 && deg == 0)
    return launch_fused_kd<3, 0>(scatter, a, fb, stream);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_ev_patch_fused_lowdeg(int k, int deg, const SeArgs& a, const FusedBins& fb, hipStream_t stream)
{
  if (k == 2 && deg == 0)
    return launch_ev_fused_kd<2, 0>(a, fb, stream);
  if (k == 3 && deg == 1)
    return launch_ev_fused_kd<3, 1>(a, fb, stream);
  if (k == 3 && deg == 0)
    return launch_ev_fused_kd<3, 0>(a, fb, stream);
  return EQLB_ERR_UNSUPPORTED;
}

int launch_se_patch_lowdeg(int k, int deg, int P, int solver, int scatter, const SeArgs& a, hipStream_t stream,
                           int mode)
{
  if (k == 4)
    return launch_se_patch_k4_lowdeg(deg, P, solver, scatter, a, stream, mode);
  if (mode != 0)
    return EQLB_ERR_UNSUPPORTED; // k <= 3: the EV patch problems run on the fused / tiled launches
  if (k == 2 && deg == 0)
    return launch_kd<2, 0>(P, solver, scatter, a, stream);
  if (k == 3 && deg == 1)
    return launch_kd<3, 1>(P, solver, scatter, a, stream);
  if (k == 3 && deg == 0)
    return launch_kd<3, 0>(P, solver, scatter, a, stream);
  return EQLB_ERR_UNSUPPORTED;
}

} // namespace eqlb
