// The kernel of eqlb_primal_flux.hip, which includes this file three times:
//   EQLB_FLUX_MU 0, EQLB_FLUX_TENSOR 0  k_primal_flux<P, D, STRESS>: the flux of a P_p solution, or the stress of a
//                                       displacement
//   EQLB_FLUX_MU 1, EQLB_FLUX_TENSOR 0  k_primal_stress_mu<P, D>: the stress times the cell-wise shear modulus of `sx`
//   EQLB_FLUX_MU 0, EQLB_FLUX_TENSOR 1  k_primal_flux_tensor<P, D>: the flux -kappa D grad u_h with the cell-wise tensor
//                                       of `tx`
#if EQLB_FLUX_TENSOR
template <int P, int D>
__global__ void __launch_bounds__(PF_THREADS)
k_primal_flux_tensor(int32_t ncells, int32_t nrhs, int64_t ndofs, const int32_t* __restrict__ cell_dofs,
                     const double* __restrict__ u, const double* __restrict__ cellJ, const double* __restrict__ coeff,
                     double pi_1, const PrimalOp<P, D> op, double* __restrict__ out, const FluxTensorArgs tx)
{
  constexpr bool STRESS = false;
#elif EQLB_FLUX_MU
template <int P, int D>
__global__ void __launch_bounds__(PF_THREADS)
k_primal_stress_mu(int32_t ncells, int32_t nrhs, int64_t ndofs, const int32_t* __restrict__ cell_dofs,
                   const double* __restrict__ u, const double* __restrict__ cellJ, const double* __restrict__ coeff,
                   double pi_1, const PrimalOp<P, D> op, double* __restrict__ out, const StressMuArgs sx)
{
  constexpr bool STRESS = true;
#else
template <int P, int D, bool STRESS>
__global__ void __launch_bounds__(PF_THREADS)
k_primal_flux(int32_t ncells, int32_t nrhs, int64_t ndofs, const int32_t* __restrict__ cell_dofs,
              const double* __restrict__ u, const double* __restrict__ cellJ, const double* __restrict__ coeff,
              double pi_1, const PrimalOp<P, D> op, double* __restrict__ out)
{
#endif
  constexpr int NP = nd_of(P), ND = nd_of(D), ROW = 2 * ND, S = ROW + 1;
  constexpr int NBUF = (PF_THREADS * S > (PF_THREADS * NP + 1) / 2) ? PF_THREADS * S : (PF_THREADS * NP + 1) / 2;
  __shared__ double sPG[2 * ND * NP];
  __shared__ double sbuf[NBUF]; // first the index rows of the workgroup, then its output rows
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * PF_THREADS;
  const int nloc = (ncells - base < PF_THREADS) ? (int)(ncells - base) : PF_THREADS;
  const bool active = t < nloc;
  for (int i = t; i < 2 * ND * NP; i += PF_THREADS)
    sPG[i] = op.v[i];
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
  double K00 = 0.0, K01 = 0.0, K10 = 0.0, K11 = 0.0, kap = 1.0;
  if (active)
  {
    const double2* Jp = reinterpret_cast<const double2*>(cellJ + 4 * (base + t));
    const double2 r0 = Jp[0], r1 = Jp[1]; // J00 J01 | J10 J11
#if EQLB_FLUX_TENSOR
    // (the statement of this variant rounds the two products of the determinant on their own)
    double idet;
    {
#pragma clang fp contract(off)
      idet = 1.0 / (r0.x * r1.y - r0.y * r1.x);
    }
#else
    const double idet = 1.0 / (r0.x * r1.y - r0.y * r1.x);
#endif
    K00 = r1.y * idet;
    K01 = -r0.y * idet;
    K10 = -r1.x * idet;
    K11 = r0.x * idet;
    if (coeff)
      kap = coeff[base + t];
    else if constexpr (STRESS)
      kap = pi_1;
  }
#if EQLB_FLUX_TENSOR
  double d00 = 1.0, d01 = 0.0, d11 = 1.0;
  if (active)
  {
    const double* Dp = tx.cell_D + 3 * (base + t);
    d00 = Dp[0];
    d01 = Dp[1];
    d11 = Dp[2];
  }
#endif
  const double bad = __longlong_as_double(0x7ff8000000000000ll);
  __syncthreads(); // the index rows are in registers: sbuf takes the output rows
  if constexpr (!STRESS)
  {
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
          double g[2];
#pragma unroll
          for (int X = 0; X < 2; ++X)
          {
            double tt[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i)
              tt[i] = __dmul_rn(sPG[(X * ND + n) * NP + i], uu[i]);
            g[X] = sorted_sum<NP>(tt);
          }
#if EQLB_FLUX_TENSOR
          // grad u_h = K^T g, then one 2 x 2 product with D and the factor -kappa: every product and every sum rounded
          // on its own (contraction is switched off for this block; the rounding intrinsics alone do not keep the
          // compiler from fusing their results)
          double f0, f1;
          {
#pragma clang fp contract(off)
            const double gx = K00 * g[0] + K10 * g[1], gy = K01 * g[0] + K11 * g[1];
            f0 = -kap * (d00 * gx + d01 * gy);
            f1 = -kap * (d01 * gx + d11 * gy);
          }
#else
          const double f0 = -kap * (K00 * g[0] + K10 * g[1]), f1 = -kap * (K01 * g[0] + K11 * g[1]);
#endif
          sbuf[t * S + 2 * n] = ok ? f0 : bad;
          sbuf[t * S + 2 * n + 1] = ok ? f1 : bad;
        }
      }
      __syncthreads();
      double* o = out + ((int64_t)r * ncells + base) * ROW;
      for (int e = t; e < nloc * ROW; e += PF_THREADS)
        o[e] = sbuf[(e / ROW) * S + (e % ROW)];
      __syncthreads();
    }
  }
  else
  {
    double val[2][ROW]; // rows of -sigma
    if (active)
    {
      double uu[2][NP];
#pragma unroll
      for (int i = 0; i < NP; ++i)
      {
        const double2 w = ok ? reinterpret_cast<const double2*>(u)[idx[i]] : make_double2(0.0, 0.0);
        uu[0][i] = w.x;
        uu[1][i] = w.y;
      }
#pragma unroll
      for (int n = 0; n < ND; ++n)
      {
        double gu[2][2]; // gu[r][d] = d_d u_r
#pragma unroll
        for (int r = 0; r < 2; ++r)
        {
          double g[2];
#pragma unroll
          for (int X = 0; X < 2; ++X)
          {
            double tt[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i)
              tt[i] = __dmul_rn(sPG[(X * ND + n) * NP + i], uu[r][i]);
            g[X] = sorted_sum<NP>(tt);
          }
          gu[r][0] = K00 * g[0] + K10 * g[1];
          gu[r][1] = K01 * g[0] + K11 * g[1];
        }
        const double ld = kap * (gu[0][0] + gu[1][1]), sh = gu[0][1] + gu[1][0];
#if EQLB_FLUX_MU
        // mu_T times the value without the term, one rounding on top of it
        const double mu = sx.cell_mu ? sx.cell_mu[base + t] : sx.mu;
        val[0][2 * n] = ok ? __dmul_rn(mu, -(2.0 * gu[0][0] + ld)) : bad;
        val[0][2 * n + 1] = ok ? __dmul_rn(mu, -sh) : bad;
        val[1][2 * n] = ok ? __dmul_rn(mu, -sh) : bad;
        val[1][2 * n + 1] = ok ? __dmul_rn(mu, -(2.0 * gu[1][1] + ld)) : bad;
#else
        val[0][2 * n] = ok ? -(2.0 * gu[0][0] + ld) : bad;
        val[0][2 * n + 1] = ok ? -sh : bad;
        val[1][2 * n] = ok ? -sh : bad;
        val[1][2 * n + 1] = ok ? -(2.0 * gu[1][1] + ld) : bad;
#endif
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
    {
      if (active)
      {
#pragma unroll
        for (int j = 0; j < ROW; ++j)
          sbuf[t * S + j] = val[r][j];
      }
      __syncthreads();
      double* o = out + ((int64_t)r * ncells + base) * ROW;
      for (int e = t; e < nloc * ROW; e += PF_THREADS)
        o[e] = sbuf[(e / ROW) * S + (e % ROW)];
      __syncthreads();
    }
  }
}
