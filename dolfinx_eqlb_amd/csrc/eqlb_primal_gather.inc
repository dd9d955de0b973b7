// The sum pass of the store-and-sum operator (eqlb_primal_common.h), included once per variant:
//   EQLB_GATHER_FACET 0  k_primal_gather        the owner sum
//   EQLB_GATHER_FACET 1  k_primal_gather_facet  the owner sum, then the facet values of the handle's facet term of the
//                        rows that lie in a listed facet, in ascending facet id, each by one addition, before b_extra,
//                        the mask, r = b - v and the inner product.  A kernel of its own with an argument the other does
//                        not take (FacetTermArgs), so that a handle without the term launches the symbol, the arguments
//                        and the code it launched before the term existed.  BS says which term it is:
//                          BS = 1  the Robin term of a scalar space (include/eqlb.h: eqlb_primal_set_robin): row e gets
//                                  w_f sum_j FacetMass[i][j] u[dof_j]; 1 or MANY_R columns
//                          BS = 2  the spring term of a blocked space, one column (eqlb_elasticity_set_springs): row
//                                  e = 2 d + r gets t_f[i][r] = Kw[r][0] m[i][0] + Kw[r][1] m[i][1] with
//                                  m[i][s] = sum_j FacetMass[i][j] u[2 dof_j + s]
//                        The table runs over the scalar DOFs d, since all rows of a DOF lie in the same facets: a chunk
//                        of PS_THREADS rows e is PS_THREADS / BS DOFs, and the lanes of a DOF find the same piece of it.
// A row finds its facets through the table of FacetTermArgs: the rows of a grid-stride step of a block are one chunk of
// PS_THREADS consecutive rows, and chunk[] says where the chunk's DOFs start in the sorted list of listed DOFs - one
// wave-uniform read per chunk.  Only a chunk that holds a listed DOF searches (bisection inside its piece of the list).
#if EQLB_GATHER_FACET
#define EQLB_GATHER_NAME k_primal_gather_facet
#else
#define EQLB_GATHER_NAME k_primal_gather
#endif

// the sum pass with BS components per DOF on the live columns: e = BS d + r runs over the blocked vectors, y_loc holds
// BS values per (cell, local index), the component fastest.  The slot range of a DOF is found once; the sum of a
// column runs in the order of the slot list
template <int BS, int NC>
__global__ void __launch_bounds__(PS_THREADS) EQLB_GATHER_NAME(const GatherArgs a
#if EQLB_GATHER_FACET
                                                               ,
                                                               const FacetTermArgs rx
#endif
)
{
#pragma clang fp contract(off)
  static_assert(BS == 1 || NC == 1, "columns for scalar spaces only");
#if EQLB_GATHER_FACET
  static_assert(BS == 1 || BS == 2, "a Robin term (BS = 1) or a spring term (BS = 2)");
#endif
  __shared__ double sh[NC][PS_THREADS];
  const uint32_t live = cols_live<NC>(a.cols);
  if (!live)
    return;
  const SpaceArgs& s = a.s;
  const int t = threadIdx.x;
  const int64_t nshared = (int64_t)s.nnodes + (int64_t)s.nfacets * s.ne, n = s.ndofs * BS;
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k)
    acc[k] = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * PS_THREADS + t; e < n; e += (int64_t)gridDim.x * PS_THREADS)
  {
    const int64_t d = e / BS;
    const int r = (int)(e - d * BS);
    int64_t beg = 0;
    int cnt = 0;
    if (d < nshared)
      slot_range(s, d, beg, cnt);
    else
    {
      const int64_t q = d - nshared, c = q / s.ni;
      beg = c * s.nd + 3 + 3 * s.ne + (q - c * s.ni); // (the one entry of an interior DOF)
    }
#if EQLB_GATHER_FACET
    // the piece of rows[] of this chunk: read here, looked at behind the owner sum, so that the wave-uniform reads
    // travel beside the reads of the sum and not in front of them
    const int ch = __builtin_amdgcn_readfirstlane((int)((e - t) / PS_THREADS));
    const int c0 = rx.chunk[ch], c1 = rx.chunk[ch + 1];
    int rb = -1, re = -1; // the entries [rb, re) of DOF d in rx.ent; rb < 0: not looked up yet, and none so far
#endif
    bool fx = false;
    if constexpr (NC > 1)
      fx = a.fixed && a.fixed[e]; // (once for the columns; the one-column instance asks behind its sum)
#pragma unroll
    for (int k = 0; k < NC; ++k)
    {
      if (!col_on<NC>(live, k))
        continue;
      const double* yl = a.yloc + k * a.ystride;
      double v;
      if (d < nshared)
      {
        v = cnt > 0 ? yl[(int64_t)s.slots[beg] * BS + r] : 0.0;
        for (int j = 1; j < cnt; ++j)
          v = v + yl[(int64_t)s.slots[beg + j] * BS + r];
      }
      else
        v = yl[beg * BS + r];
#if EQLB_GATHER_FACET
      if (c1 > c0 && rb < 0)
      {
        int lo = c0, hi = c1;
        while (lo < hi)
        {
          const int mid = (lo + hi) >> 1;
          if (rx.rows[mid] < d)
            lo = mid + 1;
          else
            hi = mid;
        }
        rb = re = 0;
        if (lo < c1 && rx.rows[lo] == d)
        {
          rb = rx.off[lo];
          re = rx.off[lo + 1];
        }
      }
      for (int q = rb; q < re; ++q)
      {
        const int32_t en = rx.ent[q];
        const int i = en & 7;
        const int64_t li = en >> 3;
        const int32_t* dd = rx.dofs + li * FACET_ROW;
        double tv;
        if constexpr (BS == 2)
        {
          const double* kw = rx.w + 3 * li; // row r of Kw: (kw[r], kw[r + 1])
          if (!rx.u)
            tv = kw[2 * r] * rx.fm[i * rx.n1 + i]; // (the diagonal: Kw[r][r])
          else
          {
            double m0 = 0.0, m1 = 0.0;
            for (int j = 0; j < rx.n1; ++j)
            {
              const int64_t ej = 2 * (int64_t)dd[j];
              const double f = rx.fm[i * rx.n1 + j];
              const double u0 = (rx.only_fixed && !rx.fixed[ej]) ? 0.0 : rx.u[ej];
              const double u1 = (rx.only_fixed && !rx.fixed[ej + 1]) ? 0.0 : rx.u[ej + 1];
              const double p0 = f * u0, p1 = f * u1;
              m0 = j == 0 ? p0 : m0 + p0;
              m1 = j == 0 ? p1 : m1 + p1;
            }
            tv = kw[r] * m0 + kw[r + 1] * m1;
          }
          v = v + tv;
        }
        else
        {
          if (!rx.u)
            tv = rx.fm[i * rx.n1 + i]; // (the diagonal)
          else
          {
            const double* uk = rx.u + k * n;
            tv = 0.0;
            for (int j = 0; j < rx.n1; ++j)
            {
              const int32_t dj = dd[j];
              const double uj = (rx.only_fixed && !rx.fixed[dj]) ? 0.0 : uk[dj];
              const double pr = rx.fm[i * rx.n1 + j] * uj;
              tv = j == 0 ? pr : tv + pr;
            }
          }
          v = v + rx.w[li] * tv;
        }
      }
#endif
      const int64_t x = k * n + e;
      if constexpr (NC == 1)
      {
        if (a.add)
          v = v + a.add[x];
        fx = a.fixed && a.fixed[e];
      }
      const double yv = fx ? 0.0 : v;
      if (a.y)
        a.y[x] = yv;
      double rv = 0.0;
      if (a.r)
      {
        rv = fx ? 0.0 : a.b[x] - v;
        a.r[x] = rv;
      }
      if (a.dot == DOT_W_Y)
        acc[k] = acc[k] + a.w[x] * yv;
      else if (a.dot == DOT_R_R)
        acc[k] = acc[k] + rv * rv;
    }
  }
  if (a.dot == DOT_NONE)
    return;
#pragma unroll
  for (int k = 0; k < NC; ++k)
    sh[k][t] = acc[k];
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, NC, PS_THREADS)
  if (t < NC && col_on<NC>(live, t))
    a.part[(int64_t)(2 * t) * gridDim.x + blockIdx.x] = sh[t][0];
}
#undef EQLB_GATHER_NAME
