// The cell kernel of eqlb_primal_solve.hip, which includes this file four times inside its unnamed namespace:
//   EQLB_CELL_REACT 0, EQLB_CELL_DIFF 0  k_primal_cell<P, MODE, D, R>: the operator, the diagonal and the load of
//                                        -div(kappa grad u)
//   EQLB_CELL_REACT 1, EQLB_CELL_DIFF 0  k_primal_cell_react<P, MODE, D, R>: operator and diagonal with the reaction
//                                        term + c u
//   EQLB_CELL_REACT 0, EQLB_CELL_DIFF 1  k_primal_cell_diff<P, MODE, D, R>: operator and diagonal of
//                                        -div(kappa D grad u) with the cell-wise tensor of `dx`
//   EQLB_CELL_REACT 1, EQLB_CELL_DIFF 1  k_primal_cell_diff_react<P, MODE, D, R>: tensor and reaction term
// One source for all, and kernels of their own rather than one with a further template argument: a handle without a
// term launches the symbols it launched before the term existed, with their arguments and their code (a shared
// __device__ body that takes the arguments by reference does not give the same code: tools/isa_compare.py).
template <int P, int MODE, int D, int R>
__global__ void __launch_bounds__(PS_THREADS)
#if EQLB_CELL_REACT && EQLB_CELL_DIFF
k_primal_cell_diff_react(const CellArgs a, const ManyCols cols, int64_t ustride, int64_t ystride, const ReactArgs rx,
                         const DiffArgs dx)
#elif EQLB_CELL_DIFF
k_primal_cell_diff(const CellArgs a, const ManyCols cols, int64_t ustride, int64_t ystride, const DiffArgs dx)
#elif EQLB_CELL_REACT
k_primal_cell_react(const CellArgs a, const ManyCols cols, int64_t ustride, int64_t ystride, const ReactArgs rx)
#else
k_primal_cell(const CellArgs a, const ManyCols cols, int64_t ustride, int64_t ystride)
#endif
{
#pragma clang fp contract(off) // the statement rounds every product and every sum on its own
  constexpr int NP = nd_of(P), ND = nd_of(D), S = NP | 1;
  constexpr bool RX = EQLB_CELL_REACT != 0;
  constexpr int NTAB = (MODE == CELL_LOAD) ? NP * ND : (RX ? 4 : 3) * NP * NP;
  static_assert(eqlb_tables::Stiff<P>::ND == NP && eqlb_tables::Load<P, D>::NP == NP && eqlb_tables::Load<P, D>::ND == ND
                    && eqlb_tables::Mass<P>::ND == NP,
                "table shape");
  static_assert(R >= 1 && R <= MANY_R && (R == 1 || MODE == CELL_OPERATOR), "columns for the operator only");
  static_assert(!RX || MODE != CELL_LOAD, "the load knows no reaction term");
  static_assert(!EQLB_CELL_DIFF || MODE != CELL_LOAD, "the load knows no tensor");
  __shared__ double sT[NTAB];
  __shared__ double sbuf[PS_THREADS * S]; // first the index rows of the workgroup, then its output rows, a column at a time
#if !EQLB_CELL_REACT
  [[maybe_unused]] const ReactArgs rx{}; // (the discarded branches below name it)
#endif
  const uint32_t live = cols_live<R>(cols);
  if (!live)
    return;
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * PS_THREADS;
  const int nloc = (a.ncells - base < PS_THREADS) ? (int)(a.ncells - base) : PS_THREADS;
  const bool active = t < nloc;
  for (int i = t; i < NTAB; i += PS_THREADS)
  {
    if constexpr (MODE == CELL_LOAD)
      sT[i] = eqlb_tables::Load<P, D>::LD[i];
    else if constexpr (RX)
      sT[i] = i < 3 * NP * NP ? eqlb_tables::Stiff<P>::ST[i] : eqlb_tables::Mass<P>::MS[i - 3 * NP * NP];
    else
      sT[i] = eqlb_tables::Stiff<P>::ST[i];
  }
  [[maybe_unused]] int32_t idx[NP];
  if constexpr (MODE == CELL_OPERATOR)
  {
    int32_t* sidx = reinterpret_cast<int32_t*>(sbuf);
    const int32_t* rows = a.cell_dofs + base * NP;
    for (int e = t; e < nloc * NP; e += PS_THREADS)
      sidx[e] = rows[e];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; ++i)
      idx[i] = active ? sidx[t * NP + i] : 0;
  }
  __syncthreads(); // the table is staged; the index rows are in registers: sbuf takes the output rows
  [[maybe_unused]] double out[R > 1 ? R : 1][R > 1 ? NP : 1];
  if constexpr (R > 1)
  {
#pragma unroll
    for (int c = 0; c < R; ++c)
#pragma unroll
      for (int i = 0; i < NP; ++i)
        out[c][i] = 0.0;
  }
  if (active)
  {
    const double2* Jp = reinterpret_cast<const double2*>(a.cellJ + 4 * (base + t));
    const double2 r0 = Jp[0], r1 = Jp[1]; // J00 J01 | J10 J11
    const double det = r0.x * r1.y - r0.y * r1.x;
    const double adet = fabs(det);
    if constexpr (MODE == CELL_LOAD)
    {
      const double* f = a.u + (base + t) * ND;
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
        sbuf[t * S + i] = adet * s;
      }
    }
    else
    {
      const double idet = 1.0 / det;
      const double K00 = r1.y * idet, K01 = -r0.y * idet, K10 = -r1.x * idet, K11 = r0.x * idet;
#if EQLB_CELL_DIFF
      // C = K D K^T with D = (d00 d01; d01 d11) of the cell: T = K D, then C_XY = T[X][0] K[Y][0] + T[X][1] K[Y][1]
      const double* Dp = dx.cell_D + 3 * (base + t);
      const double d00 = Dp[0], d01 = Dp[1], d11 = Dp[2];
      const double T00 = K00 * d00 + K01 * d01, T01 = K00 * d01 + K01 * d11;
      const double T10 = K10 * d00 + K11 * d01, T11 = K10 * d01 + K11 * d11;
      const double C00 = T00 * K00 + T01 * K01, C01 = T00 * K10 + T01 * K11, C11 = T10 * K10 + T11 * K11;
#else
      const double C00 = K00 * K00 + K01 * K01, C01 = K00 * K10 + K01 * K11, C11 = K10 * K10 + K11 * K11;
#endif
      const double w = (a.coeff ? a.coeff[base + t] : 1.0) * adet;
      [[maybe_unused]] double wm = 0.0;
      if constexpr (RX)
        wm = (rx.cell_c ? rx.cell_c[base + t] : rx.c) * adet;
      [[maybe_unused]] double uu[R][NP];
      if constexpr (MODE == CELL_OPERATOR)
      {
#pragma unroll
        for (int i = 0; i < NP; ++i)
        {
          const bool zero = a.only_fixed && !a.fixed[idx[i]];
#pragma unroll
          for (int c = 0; c < R; ++c)
          {
            const double v = col_on<R>(live, c) ? a.u[c * ustride + idx[i]] : 0.0;
            uu[c][i] = zero ? 0.0 : v;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NP; ++i)
      {
        double tm[R][3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
        {
          const double* row = sT + (m * NP + i) * NP;
          if constexpr (MODE == CELL_DIAGONAL)
            tm[0][m] = row[i];
          else
          {
            double s[R];
            {
              const double e = row[0];
#pragma unroll
              for (int c = 0; c < R; ++c)
                s[c] = e * uu[c][0];
            }
#pragma unroll
            for (int j = 1; j < NP; ++j)
            {
              const double e = row[j];
#pragma unroll
              for (int c = 0; c < R; ++c)
                s[c] = s[c] + e * uu[c][j];
            }
#pragma unroll
            for (int c = 0; c < R; ++c)
              tm[c][m] = s[c];
          }
        }
        [[maybe_unused]] double ms[R];
        if constexpr (RX)
        {
          const double* row = sT + (3 * NP + i) * NP;
          if constexpr (MODE == CELL_DIAGONAL)
            ms[0] = row[i];
          else
          {
            {
              const double e = row[0];
#pragma unroll
              for (int c = 0; c < R; ++c)
                ms[c] = e * uu[c][0];
            }
#pragma unroll
            for (int j = 1; j < NP; ++j)
            {
              const double e = row[j];
#pragma unroll
              for (int c = 0; c < R; ++c)
                ms[c] = ms[c] + e * uu[c][j];
            }
          }
        }
#pragma unroll
        for (int c = 0; c < R; ++c)
        {
          double v = w * ((C00 * tm[c][0] + C01 * tm[c][1]) + C11 * tm[c][2]);
          if constexpr (RX)
            v = v + wm * ms[c];
          if constexpr (R == 1)
            sbuf[t * S + i] = v;
          else
            out[c][i] = v;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < R; ++c)
  {
    if (!col_on<R>(live, c)) // (the same in every thread)
      continue;
    if constexpr (R > 1)
    {
      if (active)
      {
#pragma unroll
        for (int i = 0; i < NP; ++i)
          sbuf[t * S + i] = out[c][i];
      }
    }
    __syncthreads();
    double* o = a.yloc + c * ystride + base * NP;
    for (int e = t; e < nloc * NP; e += PS_THREADS)
      o[e] = sbuf[(e / NP) * S + (e % NP)];
    if constexpr (R > 1)
      __syncthreads(); // (the next column overwrites sbuf)
  }
}
