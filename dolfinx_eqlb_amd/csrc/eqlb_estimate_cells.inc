// The cell kernel of eqlb_estimate_kernels.h, which includes this file twice:
//   EQLB_EST_WEIGHTED 0  k_estimate_cells<K, DEG>: divergence residual and flux norm
//   EQLB_EST_WEIGHTED 1  k_estimate_cells_weighted<K, DEG>: the flux norm weighted by W = adj(D) / (kappa det D) of `wx`
// one thread per cell
template <int K, int DEG>
__global__ void __launch_bounds__(256)
#if EQLB_EST_WEIGHTED
k_estimate_cells_weighted(int32_t ncells, const double* __restrict__ tab, const double* __restrict__ cellJ,
                          const double* __restrict__ x_eq, const double* __restrict__ flux_dg,
                          double* __restrict__ sig2, const double alpha, const EstWeightArgs wx)
#else
k_estimate_cells(int32_t ncells, const double* __restrict__ tab, const double* __restrict__ cellJ,
                 const double* __restrict__ x_eq, const double* __restrict__ flux_dg,
                 const double* __restrict__ rhs_dg, double* __restrict__ div2, double* __restrict__ sig2,
                 const double alpha, const double beta)
#endif
{
  using E = EstTables<K, DEG>;
#if EQLB_EST_WEIGHTED
  constexpr int NRT = E::NRT, ND = E::ND;
#else
  constexpr int NRT = E::NRT, ND = E::ND, NQ = E::NQ;
#endif
  extern __shared__ double st[];
  for (int i = threadIdx.x; i < E::TOTAL; i += 256)
    st[i] = tab[i];
  __syncthreads();
  const int32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells)
    return;
  const double* J = cellJ + 4 * (int64_t)c;
  const double J00 = J[0], J01 = J[1], J10 = J[2], J11 = J[3];
  const double detJ = J00 * J11 - J01 * J10, ia = 1.0 / fabs(detJ);
#if !EQLB_EST_WEIGHTED
  const double a00 = J11, a01 = -J01, a10 = -J10, a11 = J00; // adj = detJ * K
#endif
  const double* co = x_eq + (int64_t)c * NRT;
  double cf[NRT];
#pragma unroll
  for (int i = 0; i < NRT; ++i)
    cf[i] = co[i];
#if !EQLB_EST_WEIGHTED
  if (div2)
  {
    double m[NQ];
    // moments of the reference divergence: q = 0 from the zero-order facet DOFs (facet 1 measures the
    // outward flux, facets 0 and 2 the inward one), q >= 1 are the div DOFs themselves
    m[0] = -(-cf[0] + cf[K] - cf[2 * K]);
#pragma unroll
    for (int q = 1; q < NQ; ++q)
      m[q] = -cf[3 * K + q - 1];
    const double* G = flux_dg + (int64_t)c * ND * 2;
    const double* f = rhs_dg + (int64_t)c * ND;
#pragma unroll
    for (int i = 0; i < ND; ++i)
    {
      const double gx = G[2 * i], gy = G[2 * i + 1];
      const double h0 = beta * (a00 * gx + a01 * gy), h1 = beta * (a10 * gx + a11 * gy), fd = detJ * f[i];
      if constexpr (DEG == 0 && K >= 2)
      {
        // P0 data: div G = 0, the rows of DM are zero (RT_1 keeps the generic contraction)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          m[q] += fd * st[E::OFF_HG + i * NQ + q];
      }
      else
      {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          m[q] += fd * st[E::OFF_HG + i * NQ + q] - h0 * st[E::OFF_DM + (i * 2 + 0) * NQ + q]
                  - h1 * st[E::OFF_DM + (i * 2 + 1) * NQ + q];
      }
    }
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      double r = 0.0;
#pragma unroll
      for (int p = 0; p < NQ; ++p)
        r += st[E::OFF_GMI + q * NQ + p] * m[p];
      s += m[q] * r;
    }
    div2[c] = s * ia;
  }
#endif
  if (sig2)
  {
#if EQLB_EST_WEIGHTED
    // W = adj(D) / (kappa det D), symmetric: W00, W01, W11; without a tensor I / kappa
    double W00 = 1.0, W01 = 0.0, W11 = 1.0;
    {
      double dn = wx.cell_coeff ? wx.cell_coeff[c] : 1.0;
      if (wx.cell_D)
      {
        const double* Dp = wx.cell_D + 3 * (int64_t)c;
        const double d00 = Dp[0], d01 = Dp[1], d11 = Dp[2];
        // det D = d00 d11 - d01^2 as an accurate difference of products (Kahan, with the exact residual of the
        // rounded square): within 2 units of the last place however close D is to singular, where the plain form loses
        // the digits the anisotropy ratio takes
        const double w2 = __dmul_rn(d01, d01);
        const double det_d = __dadd_rn(__fma_rn(d00, d11, -w2), __fma_rn(-d01, d01, w2));
        dn = __dmul_rn(dn, det_d);
        W00 = d11;
        W01 = -d01;
        W11 = d00;
      }
      const double iw = 1.0 / dn;
      W00 *= iw;
      W01 *= iw;
      W11 *= iw;
    }
    // the metric J^T W J / |det J| in the place of J^T J / |det J|
    const double M00 = W00 * J00 + W01 * J10, M01 = W00 * J01 + W01 * J11, M10 = W01 * J00 + W11 * J10,
                 M11 = W01 * J01 + W11 * J11;
    const double g0 = (J00 * M00 + J10 * M10) * ia, g1 = (J00 * M01 + J10 * M11) * ia,
                 g2 = (J01 * M01 + J11 * M11) * ia;
#else
    const double g0 = (J00 * J00 + J10 * J10) * ia, g1 = (J00 * J01 + J10 * J11) * ia,
                 g2 = (J01 * J01 + J11 * J11) * ia;
#endif
    double s = 0.0;
    // The loops over the rows of S (and of MRD below) are unrolled in full at d < k - 1, so that cf stays in
    // registers.  The d = k - 1 instances keep the loop the compiler makes of it (RT_4 / DG_3 indexes cf in 208 B
    // of scratch): their code is left as it was, hence the two copies.
    if constexpr (DEG == K - 1)
    {
      for (int i = 0; i < NRT; ++i)
      {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < NRT; ++j)
          r += (g0 * st[E::OFF_S + i * NRT + j] + g1 * st[E::OFF_S + (NRT + i) * NRT + j]
                + g2 * st[E::OFF_S + (2 * NRT + i) * NRT + j])
               * cf[j];
        s += cf[i] * r;
      }
    }
    else
    {
#pragma unroll
      for (int i = 0; i < NRT; ++i)
      {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < NRT; ++j)
          r += (g0 * st[E::OFF_S + i * NRT + j] + g1 * st[E::OFF_S + (NRT + i) * NRT + j]
                + g2 * st[E::OFF_S + (2 * NRT + i) * NRT + j])
               * cf[j];
        s += cf[i] * r;
      }
    }
    // S1 holds phi_i^x phi_j^y + phi_i^y phi_j^x, so c^T S1 c counts the mixed term twice as needed
    if (alpha != 0.0)
    {
      // || sigma + alpha G ||^2 = || sigma ||^2 + 2 alpha (sigma, G) + alpha^2 (G, G)
      const double sg = (detJ > 0.0) ? 1.0 : -1.0;
      const double* G = flux_dg + (int64_t)c * ND * 2;
      double sgm = 0.0, gg = 0.0;
#pragma unroll
      for (int d = 0; d < ND; ++d)
      {
#if EQLB_EST_WEIGHTED
        const double hx = G[2 * d], hy = G[2 * d + 1];
        const double gx = W00 * hx + W01 * hy, gy = W01 * hx + W11 * hy; // W G_d: J^T W G_d and G_d^T W G_e below
#else
        const double gx = G[2 * d], gy = G[2 * d + 1];
#endif
        const double t0 = J00 * gx + J10 * gy, t1 = J01 * gx + J11 * gy; // J^T G_d
        if constexpr (DEG == K - 1)
        {
          for (int i = 0; i < NRT; ++i)
            sgm += cf[i] * (st[E::OFF_MRD + (i * ND + d) * 2] * t0 + st[E::OFF_MRD + (i * ND + d) * 2 + 1] * t1);
        }
        else
        {
#pragma unroll
          for (int i = 0; i < NRT; ++i)
            sgm += cf[i] * (st[E::OFF_MRD + (i * ND + d) * 2] * t0 + st[E::OFF_MRD + (i * ND + d) * 2 + 1] * t1);
        }
#pragma unroll
        for (int e = 0; e < ND; ++e)
          gg += st[E::OFF_MPS + d * ND + e] * (gx * G[2 * e] + gy * G[2 * e + 1]);
      }
      s += 2.0 * alpha * sg * sgm + alpha * alpha * fabs(detJ) * gg;
    }
    sig2[c] = s;
  }
}
