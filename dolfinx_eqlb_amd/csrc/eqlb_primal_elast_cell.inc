// The cell kernel of eqlb_primal_elasticity.hip, which includes this file four times inside its unnamed namespace:
//   EQLB_CELL_REACT 0, EQLB_CELL_SHEAR 0  k_elast_cell<P, MODE, D>: the operator, the diagonal and the load of
//                                         -div(2 eps(u) + pi_1 div(u) I)
//   EQLB_CELL_REACT 1, EQLB_CELL_SHEAR 0  k_elast_cell_react<P, MODE, D>: operator and diagonal with the reaction term + c u
//   EQLB_CELL_REACT 0, EQLB_CELL_SHEAR 1  k_elast_cell_shear<P, MODE, D>: operator and diagonal of
//                                         -div(mu (2 eps(u) + pi_1 div(u) I)), mu_T per cell
//   EQLB_CELL_REACT 1, EQLB_CELL_SHEAR 1  k_elast_cell_react_shear<P, MODE, D>: both terms
// One source for all, and separate kernels rather than one with further template arguments: a handle without a term
// launches the symbols it launched before the term existed, with their arguments and their code (a shared __device__
// body that takes the arguments by reference does not give the same code: tools/isa_compare.py).
template <int P, int MODE, int D>
__global__ void __launch_bounds__(ES_THREADS)
#if EQLB_CELL_REACT && EQLB_CELL_SHEAR
k_elast_cell_react_shear(const ElastCellArgs a, const ReactArgs rx, const ShearArgs sx)
#elif EQLB_CELL_SHEAR
k_elast_cell_shear(const ElastCellArgs a, const ShearArgs sx)
#elif EQLB_CELL_REACT
k_elast_cell_react(const ElastCellArgs a, const ReactArgs rx)
#else
k_elast_cell(const ElastCellArgs a)
#endif
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  constexpr int NP = nd_of(P), ND = nd_of(D), W = 2 * NP, S = W | 1, NN = NP * NP;
  constexpr bool RX = EQLB_CELL_REACT != 0, SH = EQLB_CELL_SHEAR != 0;
  constexpr int NTAB = (MODE == CELL_LOAD) ? NP * ND : (RX ? 4 : 3) * NN;
  static_assert(eqlb_tables::Stiff<P>::ND == NP && eqlb_tables::Cross<P>::ND == NP && eqlb_tables::Load<P, D>::NP == NP
                    && eqlb_tables::Load<P, D>::ND == ND && eqlb_tables::Mass<P>::ND == NP,
                "table shape");
  static_assert(!(RX || SH) || MODE != CELL_LOAD, "the load knows neither the reaction term nor the shear modulus");
  __shared__ double sT[NTAB];
  __shared__ double sbuf[ES_THREADS * S]; // first the index rows of the workgroup, then its output rows
#if !EQLB_CELL_REACT
  [[maybe_unused]] const ReactArgs rx{}; // (the discarded branches below name it)
#endif
#if !EQLB_CELL_SHEAR
  [[maybe_unused]] const ShearArgs sx{};
#endif
  if (a.st && a.st->done)
    return;
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * ES_THREADS;
  const int nloc = (a.ncells - base < ES_THREADS) ? (int)(a.ncells - base) : ES_THREADS;
  const bool active = t < nloc;
  for (int i = t; i < NTAB; i += ES_THREADS)
  {
    if constexpr (MODE == CELL_LOAD)
      sT[i] = eqlb_tables::Load<P, D>::LD[i];
    else if constexpr (RX) // S0 | S2 | Cross | Mass
      sT[i] = i < NN ? eqlb_tables::Stiff<P>::ST[i]
                     : i < 2 * NN ? eqlb_tables::Stiff<P>::ST[NN + i]
                                  : i < 3 * NN ? eqlb_tables::Cross<P>::CR[i - 2 * NN] : eqlb_tables::Mass<P>::MS[i - 3 * NN];
    else // S0 | S2 | Cross
      sT[i] = i < NN ? eqlb_tables::Stiff<P>::ST[i]
                     : i < 2 * NN ? eqlb_tables::Stiff<P>::ST[NN + i] : eqlb_tables::Cross<P>::CR[i - 2 * NN];
  }
  [[maybe_unused]] int32_t idx[NP];
  if constexpr (MODE == CELL_OPERATOR)
  {
    int32_t* sidx = reinterpret_cast<int32_t*>(sbuf);
    const int32_t* rows = a.cell_dofs + base * NP;
    for (int e = t; e < nloc * NP; e += ES_THREADS)
      sidx[e] = rows[e];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; ++i)
      idx[i] = active ? sidx[t * NP + i] : 0;
  }
  __syncthreads(); // the table is staged; the index rows are in registers: sbuf takes the output rows
  if (active)
  {
    const double2* Jp = reinterpret_cast<const double2*>(a.cellJ + 4 * (base + t));
    const double2 r0 = Jp[0], r1 = Jp[1]; // J00 J01 | J10 J11
    const double det = r0.x * r1.y - r0.y * r1.x;
    const double adet = fabs(det);
    if constexpr (MODE == CELL_LOAD)
    {
#pragma unroll
      for (int r = 0; r < 2; ++r)
      {
        const double* f = a.u + ((int64_t)r * a.ncells + base + t) * ND;
        double fv[ND];
#pragma unroll
        for (int n = 0; n < ND; ++n)
          fv[n] = f[n];
#pragma unroll
        for (int i = 0; i < NP; ++i)
        {
          double s = sT[i * ND] * fv[0];
#pragma unroll
          for (int n = 1; n < ND; ++n)
            s = s + sT[i * ND + n] * fv[n];
          sbuf[t * S + 2 * i + r] = adet * s;
        }
      }
    }
    else
    {
      const double idet = 1.0 / det;
      const double K[2][2] = {{r1.y * idet, -r0.y * idet}, {-r1.x * idet, r0.x * idet}}; // K[X][d]
      double Q[2][2][4];
#pragma unroll
      for (int aa = 0; aa < 2; ++aa)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
          for (int X = 0; X < 2; ++X)
#pragma unroll
            for (int Y = 0; Y < 2; ++Y)
              Q[aa][bb][2 * X + Y] = K[X][aa] * K[Y][bb];
      const double pi = a.cell_pi1 ? a.cell_pi1[base + t] : a.pi_1;
      [[maybe_unused]] double wm = 0.0;
      if constexpr (RX)
        wm = (rx.cell_c ? rx.cell_c[base + t] : rx.c) * adet;
      [[maybe_unused]] double mu = 1.0;
      if constexpr (SH)
        mu = sx.cell_mu ? sx.cell_mu[base + t] : sx.mu;
      [[maybe_unused]] double uu[2][NP];
      if constexpr (MODE == CELL_OPERATOR)
      {
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
          for (int r = 0; r < 2; ++r)
          {
            const int64_t e = 2 * (int64_t)idx[i] + r;
            const double v = a.u[e];
            uu[r][i] = (a.only_fixed && !a.fixed[e]) ? 0.0 : v;
          }
      }
      const double *S0 = sT, *S2 = sT + NN, *CR = sT + 2 * NN;
      [[maybe_unused]] const double* MS = sT + 3 * NN;
      // the rows are a loop from P = 3 on: unrolled, the compiler keeps table values of many rows in flight and P = 4
      // takes 256 VGPRs + 238 AGPRs; i indexes LDS only, so the loop needs no register array indexed by it
      constexpr int UNROLL_ROWS = NP <= 6 ? NP : 1;
#pragma unroll UNROLL_ROWS
      for (int i = 0; i < NP; ++i)
      {
        if constexpr (MODE == CELL_DIAGONAL)
        {
          const double g[4] = {S0[i * NP + i], CR[i * NP + i], CR[i * NP + i], S2[i * NP + i]};
          double Dd[2][2];
#pragma unroll
          for (int aa = 0; aa < 2; ++aa)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
              Dd[aa][bb] = (Q[aa][bb][0] * g[0] + Q[aa][bb][1] * g[1]) + (Q[aa][bb][2] * g[2] + Q[aa][bb][3] * g[3]);
#pragma unroll
          for (int r = 0; r < 2; ++r)
          {
            double v = adet * (((Dd[0][0] + Dd[1][1]) + Dd[r][r]) + pi * Dd[r][r]);
            if constexpr (SH) // one product on top of the value formed without the term
              v = mu * v;
            if constexpr (RX)
              v = v + wm * MS[i * NP + i];
            sbuf[t * S + 2 * i + r] = v;
          }
        }
        else
        {
          double Dd[2][2][2]; // [s][a][b]
#pragma unroll
          for (int s = 0; s < 2; ++s)
          {
            double g0 = S0[i * NP] * uu[s][0], g1 = CR[i * NP] * uu[s][0], g2 = CR[i] * uu[s][0],
                   g3 = S2[i * NP] * uu[s][0];
#pragma unroll
            for (int j = 1; j < NP; ++j)
            {
              g0 = g0 + S0[i * NP + j] * uu[s][j];
              g1 = g1 + CR[i * NP + j] * uu[s][j];
              g2 = g2 + CR[j * NP + i] * uu[s][j];
              g3 = g3 + S2[i * NP + j] * uu[s][j];
            }
#pragma unroll
            for (int aa = 0; aa < 2; ++aa)
#pragma unroll
              for (int bb = 0; bb < 2; ++bb)
                Dd[s][aa][bb] = (Q[aa][bb][0] * g0 + Q[aa][bb][1] * g1) + (Q[aa][bb][2] * g2 + Q[aa][bb][3] * g3);
          }
          double v0 = adet * (((Dd[0][0][0] + Dd[0][1][1]) + (Dd[0][0][0] + Dd[1][1][0]))
                              + pi * (Dd[0][0][0] + Dd[1][0][1]));
          double v1 = adet * (((Dd[1][0][0] + Dd[1][1][1]) + (Dd[0][0][1] + Dd[1][1][1]))
                              + pi * (Dd[0][1][0] + Dd[1][1][1]));
          if constexpr (SH) // one product on top of the value formed without the term; the reaction term is not scaled
          {
            v0 = mu * v0;
            v1 = mu * v1;
          }
          if constexpr (RX)
          {
            double m0 = MS[i * NP] * uu[0][0], m1 = MS[i * NP] * uu[1][0];
#pragma unroll
            for (int j = 1; j < NP; ++j)
            {
              m0 = m0 + MS[i * NP + j] * uu[0][j];
              m1 = m1 + MS[i * NP + j] * uu[1][j];
            }
            v0 = v0 + wm * m0;
            v1 = v1 + wm * m1;
          }
          sbuf[t * S + 2 * i] = v0;
          sbuf[t * S + 2 * i + 1] = v1;
        }
      }
    }
  }
  __syncthreads();
  double* o = a.yloc + base * W;
  for (int e = t; e < nloc * W; e += ES_THREADS)
    o[e] = sbuf[(e / W) * S + (e % W)];
}
