// The cell kernel of the stress estimator in eqlb_estimate.hip, which includes this file twice:
//   EQLB_EST_MU 0  k_estimate_stress_cells<K>: the terms in the non-dimensional form (mu = 1), one scalar pi_1
//   EQLB_EST_MU 1  k_estimate_stress_cells_mu<K>: pi_T and mu_T per cell (StressCoeffArgs); energy and wsym are the
//                  values of the kernel above, formed with pi_T, divided by mu_T
// One source and two kernels, so that eqlb_se_estimate_stress launches the symbol, arguments and code it launched before.
template <int K>
__global__ void __launch_bounds__(256)
#if EQLB_EST_MU
k_estimate_stress_cells_mu(int32_t ncells, const double* __restrict__ tab, const double* __restrict__ cellJ,
                           const double* __restrict__ x0, const double* __restrict__ x1,
                           const double* __restrict__ korn, const StressCoeffArgs co, double* __restrict__ energy,
                           double* __restrict__ wsym, double* __restrict__ asym3)
#else
k_estimate_stress_cells(int32_t ncells, const double* __restrict__ tab, const double* __restrict__ cellJ,
                        const double* __restrict__ x0, const double* __restrict__ x1,
                        const double* __restrict__ korn, const double pi_1, double* __restrict__ energy,
                        double* __restrict__ wsym, double* __restrict__ asym3)
#endif
{
  using R = eqlb_tables::Ref<K, K - 1>;
  constexpr int NRT = R::NRT, NSU = R::SU_SIZE, NV = R::V_SIZE;
  extern __shared__ double st[];
  for (int i = threadIdx.x; i < NSU + NV; i += 256)
    st[i] = tab[i];
  __syncthreads();
  const int32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells)
    return;
  const double* J = cellJ + 4 * (int64_t)c;
  const double Jm[2][2] = {{J[0], J[1]}, {J[2], J[3]}};
  const double detJ = J[0] * J[3] - J[1] * J[2], ia = 1.0 / fabs(detJ);
  double c0[NRT], c1[NRT];
#pragma unroll
  for (int i = 0; i < NRT; ++i)
  {
    c0[i] = x0[(int64_t)c * NRT + i];
    c1[i] = x1[(int64_t)c * NRT + i];
  }
  // W[t][r][s] = c_r^T SU_t c_s, t = (xx, xy, yy)
  double W[3][2][2];
#pragma unroll
  for (int t = 0; t < 3; ++t)
  {
    double w00 = 0.0, w01 = 0.0, w10 = 0.0, w11 = 0.0;
    for (int i = 0; i < NRT; ++i)
    {
      double u0 = 0.0, u1 = 0.0;
#pragma unroll
      for (int j = 0; j < NRT; ++j)
      {
        const double a = st[(t * NRT + i) * NRT + j];
        u0 += a * c0[j];
        u1 += a * c1[j];
      }
      w00 += c0[i] * u0;
      w01 += c0[i] * u1;
      w10 += c1[i] * u0;
      w11 += c1[i] * u1;
    }
    W[t][0][0] = w00;
    W[t][0][1] = w01;
    W[t][1][0] = w10;
    W[t][1][1] = w11;
  }
  // int_T sigma_r^x sigma_s^y
  auto prod = [&](int x, int y, int r, int s) {
    return ia
           * (Jm[x][0] * Jm[y][0] * W[0][r][s] + Jm[x][0] * Jm[y][1] * W[1][r][s] + Jm[x][1] * Jm[y][0] * W[1][s][r]
              + Jm[x][1] * Jm[y][1] * W[2][r][s]);
  };
  const double fro = prod(0, 0, 0, 0) + prod(1, 1, 0, 0) + prod(0, 0, 1, 1) + prod(1, 1, 1, 1);
  const double tr2 = prod(0, 0, 0, 0) + 2.0 * prod(0, 1, 0, 1) + prod(1, 1, 1, 1);
  const double as2 = prod(1, 1, 0, 0) - 2.0 * prod(1, 0, 0, 1) + prod(0, 0, 1, 1);
  const double ck = korn ? korn[c] : 1.0;
#if EQLB_EST_MU
  const double pi_1 = co.cell_pi1 ? co.cell_pi1[c] : co.pi_1, mu = co.cell_mu ? co.cell_mu[c] : co.mu;
  if (energy)
    energy[c] = __ddiv_rn(0.5 * (fro - pi_1 / (2.0 + 2.0 * pi_1) * tr2), mu);
  if (wsym)
    wsym[c] = __ddiv_rn(0.25 * ck * ck * as2, mu);
#else
  if (energy)
    energy[c] = 0.5 * (fro - pi_1 / (2.0 + 2.0 * pi_1) * tr2);
  if (wsym)
    wsym[c] = 0.25 * ck * ck * as2;
#endif
  if (asym3)
  {
    const double sg = (detJ > 0.0) ? 1.0 : -1.0;
    const double* V = st + NSU; // V[v][i][a] = int hat_v phi_i^a
#pragma unroll
    for (int v = 0; v < 3; ++v)
    {
      double r = 0.0;
      for (int i = 0; i < NRT; ++i)
      {
        const double v0 = V[(v * NRT + i) * 2], v1 = V[(v * NRT + i) * 2 + 1];
        r += c0[i] * (Jm[1][0] * v0 + Jm[1][1] * v1) - c1[i] * (Jm[0][0] * v0 + Jm[0][1] * v1);
      }
      asym3[(int64_t)c * 3 + v] = sg * r;
    }
  }
}
