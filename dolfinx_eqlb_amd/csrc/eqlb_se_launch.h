// The per-bin and fused launches of se_patch_body (eqlb_se_body.h): kernels, their launchers by template
// arguments, and the reference tensors of a (K, DEG) pair as the table a handle uploads.  The translation units
// that include this header instantiate them: eqlb_se_kernels.hip at DEG = k - 1, eqlb_se_kernels_lowdeg.hip and
// eqlb_se_kernels_lowdeg_k4.hip below.
#pragma once

#include "eqlb_se_body.h"

namespace eqlb
{

template <int K, int DEG>
static void fill_tables_t(std::vector<double>& out)
{
  using R = eqlb_tables::Ref<K, DEG>;
  out.clear();
  out.insert(out.end(), R::S, R::S + R::S_SIZE);
  out.insert(out.end(), R::F, R::F + R::F_SIZE);
  static_assert(R::H_SIZE % 3 == 0, "H holds one row per local vertex");
  for (int n = 0; n < 3; ++n) // rows padded to an even length (Sizes::HROW)
  {
    out.insert(out.end(), R::H + n * (R::H_SIZE / 3), R::H + (n + 1) * (R::H_SIZE / 3));
    if ((R::H_SIZE / 3) & 1)
      out.push_back(0.0);
  }
  out.insert(out.end(), R::D, R::D + R::D_SIZE);
  {
    using Z = Sizes<K, DEG, 8>;
    static_assert(R::TE_SIZE == NCOMBO * 3 * Z::NTE && R::WQ_SIZE == NCOMBO * 3 * Z::NH * Z::NCOL, "tensor sizes");
    for (int r = 0; r < NCOMBO * 3; ++r) // rows padded to Sizes::NTES
    {
      out.insert(out.end(), R::TE + r * Z::NTE, R::TE + (r + 1) * Z::NTE);
      out.insert(out.end(), Z::NTES - Z::NTE, 0.0);
    }
    for (int r = 0; r < NCOMBO * 3 * Z::NH; ++r) // rows padded to Sizes::NCOLS
    {
      out.insert(out.end(), R::WQ + r * Z::NCOL, R::WQ + (r + 1) * Z::NCOL);
      out.insert(out.end(), Z::NCOLS - Z::NCOL, 0.0);
    }
  }
  out.insert(out.end(), R::HB, R::HB + R::HB_SIZE);
  out.insert(out.end(), R::V, R::V + R::V_SIZE);
  out.insert(out.end(), R::VQ, R::VQ + R::VQ_SIZE);
  out.insert(out.end(), R::HG, R::HG + R::HG_SIZE);
  if (R::HG_SIZE & 1) // Sizes::NHG
    out.push_back(0.0);
  out.insert(out.end(), R::WG, R::WG + R::WG_SIZE);
}

// one bin per launch (any solver)
template <int K, int DEG, int P, int SOLVER, int SCATTER, int MODE = 0>
__global__ void __launch_bounds__((Sizes<K, DEG, P>::block_of(SOLVER)), ((K >= 4 && SOLVER == 1) ? EQLB_K4_WAVES : 1))
k_se_patch(const SeArgs a)
{
  extern __shared__ __align__(16) double lds[];
  se_patch_body<K, DEG, P, SOLVER, SCATTER, Sizes<K, DEG, P>::block_of(SOLVER), MODE>(a, blockIdx.x, lds);
}

// all bins in ONE launch (register solver): blocks [start[b], start[b+1]) run the P = 4 << b body,
// so the bins overlap on the chip and there are no launch gaps / tails between them
template <int K, int DEG, int SOLVER, int SCATTER>
__global__ void __launch_bounds__(256, (K <= 2 ? EQLB_FUSED_WAVES : 1)) k_se_patch_fused(const SeArgs a0, const FusedBins fb)
{
  // PERSISTENT workgroups: the grid is sized to the chip (launch_fused_kd), every workgroup stages
  // the reference tensors in LDS once and then strides over the 256-lane work blocks of all bins;
  // its waves drift apart (no block barrier in the loop), so gathers of one wave overlap the
  // arithmetic of the others.
  extern __shared__ __align__(16) double lds[];
  using Z = Sizes<K, DEG, 8>;
  for (int i = threadIdx.x; i < Z::NTAB; i += 256)
    lds[i] = a0.tables[Z::NS + i];
  __syncthreads();
  const int64_t nwork = fb.block_start[MAX_BINS];
  for (int64_t bid = blockIdx.x; bid < nwork; bid += gridDim.x)
  {
    int b = 0;
#pragma unroll
    for (int i = 1; i < MAX_BINS; ++i)
      if (bid >= fb.block_start[i])
        b = i;
    SeArgs a = a0;
    a.npatch = fb.npatch[b];
    a.slot_offset = fb.slot_offset[b];
    a.patch_offset = fb.patch_offset[b];
    const int64_t lb = bid - fb.block_start[b];
    switch (b)
    {
    case 0:
      se_patch_body<K, DEG, 4, SOLVER, SCATTER, 256>(a, lb, lds, true);
      break;
    case 1:
      se_patch_body<K, DEG, 8, SOLVER, SCATTER, 256>(a, lb, lds, true);
      break;
    case 2:
      se_patch_body<K, DEG, 16, SOLVER, SCATTER, 256>(a, lb, lds, true);
      break;
    case 3:
      se_patch_body<K, DEG, 32, SOLVER, SCATTER, 256>(a, lb, lds, true);
      break;
    default:
      se_patch_body<K, DEG, 64, SOLVER, SCATTER, 256>(a, lb, lds, true);
      break;
    }
  }
}

// constrained-minimisation (EV) patch problems, all bins in one launch (MODE 1 of the body)
template <int K, int DEG>
__global__ void __launch_bounds__(256, (K <= 2 ? 2 : 1)) k_ev_patch_fused(const SeArgs a0, const FusedBins fb)
{
  extern __shared__ __align__(16) double lds[];
  const int64_t bid = blockIdx.x;
  int b = 0;
#pragma unroll
  for (int i = 1; i < MAX_BINS; ++i)
    if (bid >= fb.block_start[i])
      b = i;
  SeArgs a = a0;
  a.npatch = fb.npatch[b];
  a.slot_offset = fb.slot_offset[b];
  a.patch_offset = fb.patch_offset[b];
  const int64_t lb = bid - fb.block_start[b];
  switch (b)
  {
  case 0:
    se_patch_body<K, DEG, 4, 1, 0, 256, 1>(a, lb, lds);
    break;
  case 1:
    se_patch_body<K, DEG, 8, 1, 0, 256, 1>(a, lb, lds);
    break;
  case 2:
    se_patch_body<K, DEG, 16, 1, 0, 256, 1>(a, lb, lds);
    break;
  case 3:
    se_patch_body<K, DEG, 32, 1, 0, 256, 1>(a, lb, lds);
    break;
  default:
    se_patch_body<K, DEG, 64, 1, 0, 256, 1>(a, lb, lds);
    break;
  }
}

template <int K, int DEG>
static int launch_ev_fused_kd(const SeArgs& a, const FusedBins& fb, hipStream_t stream)
{
  const size_t lds_bytes = sizeof(double) * (size_t)Sizes<K, DEG, 8>::lds_doubles(256, 1, 1);
  const int64_t grid = fb.block_start[MAX_BINS];
  if (grid == 0)
    return 0;
  hipLaunchKernelGGL((k_ev_patch_fused<K, DEG>), dim3((unsigned)grid), dim3(256), lds_bytes, stream, a, fb);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

// ---- dispatch -------------------------------------------------------------------------------------
template <int K, int DEG, int P, int SOLVER, int SCATTER, int MODE = 0>
static int launch_t(const SeArgs& a, hipStream_t stream)
{
  using Z = Sizes<K, DEG, P>;
  constexpr int BLOCK = Z::block_of(SOLVER);
  const size_t lds_bytes = sizeof(double) * (size_t)Z::lds_doubles(BLOCK, SOLVER, MODE);
  if (lds_bytes > 160 * 1024)
    return EQLB_ERR_UNSUPPORTED;
  auto kern = k_se_patch<K, DEG, P, SOLVER, SCATTER, MODE>;
  if (lds_bytes > 64 * 1024)
  {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)
        != hipSuccess)
      return EQLB_ERR_DEVICE;
  }
  const int64_t nthreads = a.npatch * P;
  const int64_t grid = (nthreads + BLOCK - 1) / BLOCK;
  if (grid == 0)
    return 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BLOCK), lds_bytes, stream, a);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

template <int K, int DEG, int SOLVER, int SCATTER>
static int launch_p(int P, const SeArgs& a, hipStream_t stream)
{
  switch (P)
  {
  case 4:
    return launch_t<K, DEG, 4, SOLVER, SCATTER>(a, stream);
  case 8:
    return launch_t<K, DEG, 8, SOLVER, SCATTER>(a, stream);
  case 16:
    return launch_t<K, DEG, 16, SOLVER, SCATTER>(a, stream);
  case 32:
    return launch_t<K, DEG, 32, SOLVER, SCATTER>(a, stream);
  case 64:
    return launch_t<K, DEG, 64, SOLVER, SCATTER>(a, stream);
  }
  return EQLB_ERR_UNSUPPORTED;
}

template <int K, int DEG>
static int launch_kd(int P, int solver, int scatter, const SeArgs& a, hipStream_t stream)
{
  if (solver == EQLB_SOLVER_SHUFFLE)
  {
    if (scatter == EQLB_SCATTER_SLOTS)
      return launch_p<K, DEG, 1, 0>(P, a, stream);
    return launch_p<K, DEG, 1, 1>(P, a, stream);
  }
  if (scatter == EQLB_SCATTER_SLOTS)
    return launch_p<K, DEG, 0, 0>(P, a, stream);
  return launch_p<K, DEG, 0, 1>(P, a, stream);
}

template <int K, int DEG>
static int launch_fused_kd(int scatter, const SeArgs& a, const FusedBins& fb, hipStream_t stream)
{
  const size_t lds_bytes = sizeof(double) * (size_t)Sizes<K, DEG, 8>::lds_doubles(256, 1);
  const int64_t nwork = fb.block_start[MAX_BINS];
  if (nwork == 0)
    return 0;
  // persistent grid: resident workgroups of the device (occupancy x CUs), at most the work
  static int64_t resident[2] = {0, 0};
  const int si = (scatter == EQLB_SCATTER_SLOTS) ? 0 : 1;
  if (resident[si] == 0)
  {
    int dev = 0, ncu = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    const void* fn = si == 0 ? reinterpret_cast<const void*>(k_se_patch_fused<K, DEG, 1, 0>)
                             : reinterpret_cast<const void*>(k_se_patch_fused<K, DEG, 1, 1>);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds_bytes) != hipSuccess || per_cu < 1)
      per_cu = 1;
    resident[si] = (int64_t)std::max(ncu, 1) * per_cu * EQLB_PERSIST_OVERSUB;
  }
  const int64_t grid = std::min(nwork, resident[si]);
  if (scatter == EQLB_SCATTER_SLOTS)
    hipLaunchKernelGGL((k_se_patch_fused<K, DEG, 1, 0>), dim3((unsigned)grid), dim3(256), lds_bytes, stream, a, fb);
  else
    hipLaunchKernelGGL((k_se_patch_fused<K, DEG, 1, 1>), dim3((unsigned)grid), dim3(256), lds_bytes, stream, a, fb);
  return (hipGetLastError() == hipSuccess) ? 0 : EQLB_ERR_DEVICE;
}

// k = 4 (three interior unknowns per cell).  Register solver (three interior unknowns condensed per cell, 3 x 3
// blocks handed down the chain): every lanes-per-patch bin, slots or atomics.  Dense LDS Cholesky: patches of up to
// 8 facets (its tile of 52 x 52 / 2 doubles per patch and the 80 KB of RT_4 tensors fill the LDS); the only path of
// the EV patch problems at k = 4.
template <int DEG>
static int launch_k4(int P, int solver, int scatter, const SeArgs& a, hipStream_t stream, int mode)
{
  if (solver == EQLB_SOLVER_SHUFFLE && mode == 0)
  {
    if (scatter == EQLB_SCATTER_SLOTS)
      return launch_p<4, DEG, 1, 0>(P, a, stream);
    return launch_p<4, DEG, 1, 1>(P, a, stream);
  }
  if (solver == EQLB_SOLVER_SHUFFLE && mode == 1 && scatter == EQLB_SCATTER_SLOTS)
  {
    // constrained-minimisation patch problems (MODE 1 of the body) on the register solver
    switch (P)
    {
    case 4:
      return launch_t<4, DEG, 4, 1, 0, 1>(a, stream);
    case 8:
      return launch_t<4, DEG, 8, 1, 0, 1>(a, stream);
    case 16:
      return launch_t<4, DEG, 16, 1, 0, 1>(a, stream);
    case 32:
      return launch_t<4, DEG, 32, 1, 0, 1>(a, stream);
    case 64:
      return launch_t<4, DEG, 64, 1, 0, 1>(a, stream);
    }
    return EQLB_ERR_UNSUPPORTED;
  }
  if (solver != EQLB_SOLVER_LDS_CHOLESKY || (P != 4 && P != 8))
    return EQLB_ERR_UNSUPPORTED;
  if (mode == 1) // constrained-minimisation patch problems (slots only)
  {
    if (scatter != EQLB_SCATTER_SLOTS)
      return EQLB_ERR_UNSUPPORTED;
    return (P == 4) ? launch_t<4, DEG, 4, 0, 0, 1>(a, stream) : launch_t<4, DEG, 8, 0, 0, 1>(a, stream);
  }
  if (scatter == EQLB_SCATTER_SLOTS)
    return (P == 4) ? launch_t<4, DEG, 4, 0, 0>(a, stream) : launch_t<4, DEG, 8, 0, 0>(a, stream);
  return (P == 4) ? launch_t<4, DEG, 4, 0, 1>(a, stream) : launch_t<4, DEG, 8, 0, 1>(a, stream);
}

} // namespace eqlb
