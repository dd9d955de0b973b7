// Marking on the device - the step after the estimator terms in the reference's adaptive workflows
// (demo/poisson_adaptive/demo_lshape.py:196-242, demo_discont-coeff.py:339-365, elasticity_adaptive/demo_cook.py:262-295):
//   eqlb_indicator_total  cell-wise sum of the squared estimator terms (with the (sqrt a + sqrt b)^2 combination of
//                         demo/poisson/demo_error_estimation.py:115-121) and the sums over the cells
//   eqlb_mark_doerfler    the shortest list of cells, largest indicators first, whose sum exceeds theta * total
// No sort: non-negative doubles order like their 64-bit patterns, so the threshold value t is found by a radix select
// on the pattern, most significant digit first, 4 bits per pass.  A pass (k_mark_histogram) computes, over the cells
// whose pattern matches the digits fixed so far, count and fp64 sum per value of the next digit; k_mark_select walks
// the 16 buckets from the top, adds them to the sum carried from the passes above and fixes the digit where the
// running sum first exceeds the cut-off.  Prefix, carried sum and counts live in device memory (MarkState): no pass
// needs the host.  After 16 passes t is known, and the number m of cells equal to t that belong to the list; an
// ordered compaction (count per block, scan of the block counts, write) with the two channels "value > t" and
// "value == t" writes the ids in ascending order - a cell equal to t is marked iff its rank among the equals is < m.
// Every floating-point sum is made of per-thread partials in a fixed order, reduced by fixed trees: no fp atomics,
// two calls on the same input give the same bits.
#include "eqlb_device_common.h"
#include "eqlb_mesh_handle.h" // (eqlb_host_util.h)
#include "eqlb_reduce.h"
#include <cmath>

namespace eqlb
{

constexpr int MK_THREADS = 256;   // threads per block of every kernel but the scan
constexpr int MK_MAXBLOCKS = 512; // blocks of a streaming kernel; also the threads of the one-block scan
constexpr int MK_BUCKETS = 16, MK_DIGIT_BITS = 4, MK_PASSES = 64 / MK_DIGIT_BITS;
constexpr int MK_MAXTERMS = 8;

struct MarkState
{
  unsigned long long prefix; // the digits fixed so far in the high bits, zeros below; after the last pass: pattern of t
  unsigned long long nbad;   // negative or NaN indicators (counted by the first pass)
  double carried;            // sum of the cells above the range of the prefix
  long long ncarried;        // their number
  double total, cutoff;      // sum of all indicators, theta * total
  long long m;               // cells equal to t that are marked
  long long nmarked;         // ncarried + m; ncells if all are marked; -1 if nbad != 0
  int all;                   // every cell is marked (theta close to 1, or no prefix exceeds the cut-off)
};

struct TermPtrs
{
  const double* p[MK_MAXTERMS];
};

__host__ __device__ inline int mark_blocks(int64_t n)
{
  const int64_t b = (n + MK_THREADS - 1) / MK_THREADS;
  return (int)(b < MK_MAXBLOCKS ? b : MK_MAXBLOCKS);
}

// pattern of a non-negative double; -0.0 counts as 0
__device__ __forceinline__ unsigned long long mark_key(double v)
{
  return (v == 0.0) ? 0ull : (unsigned long long)__double_as_longlong(v);
}

// sum over the 16 lanes of a row of the wave; the butterfly adds the same pairs in every lane, so all 16 hold the
// same bits
__device__ __forceinline__ double row16_sum(double v)
{
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1)
    v += __shfl_xor(v, off, 16);
  return v;
}
__device__ __forceinline__ long long row16_sum(long long v)
{
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1)
    v += __shfl_xor(v, off, 16);
  return v;
}

// One pass of the radix select: psum[q][block], pcnt[q][block] = sum / number of the block's cells with digit q at
// `shift` among those that match the prefix above it (first pass: all valid cells; it also counts the invalid ones).
// The 16 buckets of a thread are updated by unrolled compare-and-select, so they stay in registers.
template <bool FIRST>
__global__ void __launch_bounds__(MK_THREADS)
k_mark_histogram(int64_t n, const double* __restrict__ eta2, int shift, MarkState* __restrict__ st,
                 double* __restrict__ psum, int* __restrict__ pcnt)
{
  __shared__ double ss[MK_BUCKETS][MK_THREADS];
  __shared__ int sc[MK_BUCKETS][MK_THREADS];
  const int t = threadIdx.x, G = gridDim.x;
  unsigned long long want = 0;
  if constexpr (!FIRST)
    want = st->prefix >> (shift + MK_DIGIT_BITS);
  double sum[MK_BUCKETS];
  int cnt[MK_BUCKETS];
#pragma unroll
  for (int q = 0; q < MK_BUCKETS; ++q)
  {
    sum[q] = 0.0;
    cnt[q] = 0;
  }
  unsigned long long nbad = 0;
  for (int64_t i = (int64_t)blockIdx.x * MK_THREADS + t; i < n; i += (int64_t)G * MK_THREADS)
  {
    const double v = eta2[i];
    const unsigned long long key = mark_key(v);
    bool use;
    if constexpr (FIRST)
    {
      use = (v >= 0.0); // false for negative values and NaN
      nbad += use ? 0 : 1;
    }
    else
      use = (key >> (shift + MK_DIGIT_BITS)) == want;
    if (use)
    {
      const int d = (int)((key >> shift) & (MK_BUCKETS - 1));
#pragma unroll
      for (int q = 0; q < MK_BUCKETS; ++q)
      {
        const bool h = (d == q);
        cnt[q] += h ? 1 : 0;
        sum[q] += h ? v : 0.0;
      }
    }
  }
  if constexpr (FIRST)
    if (nbad)
      atomicAdd(&st->nbad, nbad);
#pragma unroll
  for (int q = 0; q < MK_BUCKETS; ++q)
  {
    ss[q][t] = sum[q];
    sc[q][t] = cnt[q];
  }
  __syncthreads();
  // thread (q, j): entries j, j + 16, ... of bucket q in this order, then the tree over j
  const int q = t >> 4, j = t & 15;
  double a = 0.0;
  long long c = 0;
#pragma unroll
  for (int i = 0; i < MK_THREADS / 16; ++i)
  {
    a += ss[q][j + 16 * i];
    c += sc[q][j + 16 * i];
  }
  a = row16_sum(a);
  c = row16_sum(c);
  if (j == 0)
  {
    psum[(int64_t)q * G + blockIdx.x] = a;
    pcnt[(int64_t)q * G + blockIdx.x] = (int)c;
  }
}

// One block: bucket totals over the blocks in a fixed order, then thread 0 walks the buckets from the top.
__global__ void __launch_bounds__(MK_THREADS)
k_mark_select(int64_t n, int G, int pass, double theta, int mark_all, MarkState* __restrict__ st,
              const double* __restrict__ psum, const int* __restrict__ pcnt)
{
  __shared__ double S[MK_BUCKETS];
  __shared__ long long Cn[MK_BUCKETS];
  const int t = threadIdx.x, q = t >> 4, j = t & 15;
  double a = 0.0;
  long long c = 0;
  for (int b = j; b < G; b += 16)
  {
    a += psum[(int64_t)q * G + b];
    c += pcnt[(int64_t)q * G + b];
  }
  a = row16_sum(a);
  c = row16_sum(c);
  if (j == 0)
  {
    S[q] = a;
    Cn[q] = c;
  }
  __syncthreads();
  if (t != 0)
    return;
  if (pass == 0)
  {
    double total = 0.0;
    for (int b = 0; b < MK_BUCKETS; ++b) // small values first
      total += S[b];
    st->total = total;
    st->cutoff = theta * total;
    if (st->nbad)
    {
      st->nmarked = -1;
      return;
    }
    if (mark_all)
      st->all = 1;
  }
  if (st->nbad)
    return;
  if (!st->all)
  {
    const double cutoff = st->cutoff;
    const int shift = 64 - MK_DIGIT_BITS * (pass + 1);
    double run = st->carried, run_last = run;
    long long nc = st->ncarried, nc_last = nc;
    int chosen = -1, last = -1;
    for (int b = MK_BUCKETS - 1; b >= 0; --b)
    {
      if (Cn[b] == 0)
        continue;
      if (run + S[b] > cutoff)
      {
        chosen = b;
        break;
      }
      last = b;
      run_last = run;
      nc_last = nc;
      run += S[b];
      nc += Cn[b];
    }
    if (chosen < 0 && pass > 0 && last >= 0)
    {
      // the bucket chosen above exceeded the cut-off as one sum, its parts do not (rounding): its lowest part
      chosen = last;
      run = run_last;
      nc = nc_last;
    }
    if (chosen < 0)
      st->all = 1; // no prefix exceeds the cut-off
    else
    {
      const unsigned long long prefix = st->prefix | ((unsigned long long)chosen << shift);
      st->prefix = prefix;
      st->carried = run;
      st->ncarried = nc;
      if (pass == MK_PASSES - 1)
      {
        // ct cells equal t: the smallest j with run + j t > cutoff, all of them if there is none
        const double tv = __longlong_as_double((long long)prefix);
        const long long ct = Cn[chosen];
        long long m = ct;
        if (fma((double)ct, tv, run) > cutoff)
        {
          long long lo = 1, hi = ct;
          while (lo < hi)
          {
            const long long mid = lo + (hi - lo) / 2;
            if (fma((double)mid, tv, run) > cutoff)
              hi = mid;
            else
              lo = mid + 1;
          }
          m = lo;
        }
        st->m = m;
        st->nmarked = nc + m;
      }
    }
  }
  if (st->all)
  {
    st->prefix = 0; // every valid cell is > 0 or == 0
    st->m = n;
    st->nmarked = n;
  }
}

// cells [lo, hi) of a block of the compaction: whole tiles of MK_THREADS cells, consecutive blocks
__device__ __forceinline__ void mark_chunk(int64_t n, int G, int b, int64_t& lo, int64_t& hi)
{
  const int64_t tiles = (n + MK_THREADS - 1) / MK_THREADS, per = (tiles + G - 1) / G;
  lo = (int64_t)b * per * MK_THREADS;
  hi = lo + per * MK_THREADS;
  if (lo > n)
    lo = n;
  if (hi > n)
    hi = n;
}

__global__ void __launch_bounds__(MK_THREADS)
k_mark_count(int64_t n, const double* __restrict__ eta2, const MarkState* __restrict__ st,
             long long* __restrict__ bc /* [2][G] */)
{
  __shared__ unsigned long long tot[2];
  if (st->nbad)
    return;
  const int t = threadIdx.x, G = gridDim.x;
  if (t < 2)
    tot[t] = 0;
  __syncthreads();
  const unsigned long long tk = st->prefix;
  int64_t lo, hi;
  mark_chunk(n, G, blockIdx.x, lo, hi);
  unsigned long long ngt = 0, neq = 0;
  for (int64_t i = lo + t; i < hi; i += MK_THREADS)
  {
    const unsigned long long key = mark_key(eta2[i]);
    ngt += (key > tk) ? 1 : 0;
    neq += (key == tk) ? 1 : 0;
  }
  if (ngt)
    atomicAdd(&tot[0], ngt);
  if (neq)
    atomicAdd(&tot[1], neq);
  __syncthreads();
  if (t < 2)
    bc[(int64_t)t * G + blockIdx.x] = (long long)tot[t];
}

// One block of MK_MAXBLOCKS threads: exclusive scan of the block counts of both channels (64-bit), and the scalars
__global__ void __launch_bounds__(MK_MAXBLOCKS)
k_mark_scan(int G, const MarkState* __restrict__ st, const long long* __restrict__ bc, long long* __restrict__ off,
            int64_t* __restrict__ nmarked, double* __restrict__ eta2_total)
{
  __shared__ long long s[2][MK_MAXBLOCKS];
  const int t = threadIdx.x;
  if (t == 0)
  {
    *nmarked = st->nmarked;
    if (eta2_total)
      *eta2_total = st->total;
  }
  if (st->nbad)
    return;
  const long long v0 = (t < G) ? bc[t] : 0, v1 = (t < G) ? bc[(int64_t)G + t] : 0;
  s[0][t] = v0;
  s[1][t] = v1;
  __syncthreads();
  for (int d = 1; d < MK_MAXBLOCKS; d <<= 1)
  {
    const long long a0 = (t >= d) ? s[0][t - d] : 0, a1 = (t >= d) ? s[1][t - d] : 0;
    __syncthreads();
    s[0][t] += a0;
    s[1][t] += a1;
    __syncthreads();
  }
  if (t < G)
  {
    off[t] = s[0][t] - v0;
    off[(int64_t)G + t] = s[1][t] - v1;
  }
}

__global__ void __launch_bounds__(MK_THREADS)
k_mark_write(int64_t n, const double* __restrict__ eta2, const MarkState* __restrict__ st,
             const long long* __restrict__ off, int32_t* __restrict__ marked)
{
  __shared__ int wtot[2][MK_THREADS / 64];
  if (st->nbad)
    return;
  const int t = threadIdx.x, G = gridDim.x, w = t >> 6, lane = t & 63;
  const unsigned long long tk = st->prefix, below = (1ull << lane) - 1ull;
  const long long m = st->m;
  long long gt_before = off[blockIdx.x], eq_before = off[(int64_t)G + blockIdx.x];
  int64_t lo, hi;
  mark_chunk(n, G, blockIdx.x, lo, hi);
  for (int64_t base = lo; base < hi; base += MK_THREADS)
  {
    const int64_t i = base + t;
    bool gt = false, eq = false;
    if (i < hi)
    {
      const unsigned long long key = mark_key(eta2[i]);
      gt = key > tk;
      eq = key == tk;
    }
    const unsigned long long bg = __ballot(gt), be = __ballot(eq);
    if (lane == 0)
    {
      wtot[0][w] = __popcll(bg);
      wtot[1][w] = __popcll(be);
    }
    __syncthreads();
    long long g0 = gt_before + __popcll(bg & below), e0 = eq_before + __popcll(be & below);
    int tg = 0, te = 0;
#pragma unroll
    for (int u = 0; u < MK_THREADS / 64; ++u)
    {
      g0 += (u < w) ? wtot[0][u] : 0;
      e0 += (u < w) ? wtot[1][u] : 0;
      tg += wtot[0][u];
      te += wtot[1][u];
    }
    if (gt || (eq && e0 < m))
      marked[g0 + (e0 < m ? e0 : m)] = (int32_t)i;
    gt_before += tg;
    eq_before += te;
    __syncthreads();
  }
}

// cell_eta2 = sum of the plain terms (+ a + b + 2 sqrt(a) sqrt(b) for the last two), block partials of every term
// and of cell_eta2: part[j][block], j = nterms for cell_eta2
__global__ void __launch_bounds__(MK_THREADS)
k_indicator_total(int64_t n, int nterms, int pair, TermPtrs tp, double* __restrict__ cell_eta2,
                  double* __restrict__ part)
{
  __shared__ double sh[MK_MAXTERMS + 1][MK_THREADS];
  const int t = threadIdx.x, G = gridDim.x;
  double acc[MK_MAXTERMS + 1];
#pragma unroll
  for (int j = 0; j <= MK_MAXTERMS; ++j)
    acc[j] = 0.0;
  const int nplain = pair ? nterms - 2 : nterms;
  for (int64_t i = (int64_t)blockIdx.x * MK_THREADS + t; i < n; i += (int64_t)G * MK_THREADS)
  {
    double e = 0.0, a = 0.0, b = 0.0;
#pragma unroll
    for (int j = 0; j < MK_MAXTERMS; ++j)
      if (j < nterms)
      {
        const double v = tp.p[j][i];
        acc[j] += v;
        e += (j < nplain) ? v : 0.0;
        a = (j == nplain) ? v : a;
        b = (j == nplain + 1) ? v : b;
      }
    if (pair)
    {
      e += a;
      e += b;
      e += 2.0 * (sqrt(a) * sqrt(b));
    }
    if (cell_eta2)
      cell_eta2[i] = e;
    acc[MK_MAXTERMS] += e;
  }
  if (!part)
    return;
#pragma unroll
  for (int j = 0; j <= MK_MAXTERMS; ++j)
    sh[j][t] = acc[j];
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, MK_MAXTERMS + 1, MK_THREADS)
  if (t <= MK_MAXTERMS)
    part[(int64_t)t * G + blockIdx.x] = sh[t][0];
}

// one block: totals[j] = sum of part[j][0 .. G) by the same tree
__global__ void __launch_bounds__(MK_THREADS)
k_indicator_reduce(int G, int nterms, const double* __restrict__ part, double* __restrict__ totals)
{
  __shared__ double sh[MK_MAXTERMS + 1][MK_THREADS];
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j <= MK_MAXTERMS; ++j)
  {
    double a = 0.0;
    for (int b = t; b < G; b += MK_THREADS)
      a += part[(int64_t)j * G + b];
    sh[j][t] = a;
  }
  __syncthreads();
  EQLB_BLOCK_TREE_SUM(sh, t, MK_MAXTERMS + 1, MK_THREADS)
  if (t < nterms)
    totals[t] = sh[t][0];
  if (t == nterms)
    totals[t] = sh[MK_MAXTERMS][0];
}

// ---- work space -----------------------------------------------------------------------------------------------
// Device-memory calls take it from the stream-ordered allocator and give it back in stream order (StreamBuf): nothing
// waits.  Host-memory calls carve it out of their staging allocation.
constexpr size_t MK_WS_STATE = 256; // MarkState, padded
static_assert(sizeof(MarkState) <= MK_WS_STATE, "work space layout");
constexpr size_t MK_WS_PSUM = MK_WS_STATE, MK_WS_PCNT = MK_WS_PSUM + sizeof(double) * MK_BUCKETS * MK_MAXBLOCKS,
                 MK_WS_BC = MK_WS_PCNT + sizeof(long long) * MK_BUCKETS * MK_MAXBLOCKS / 2,
                 MK_WS_OFF = MK_WS_BC + sizeof(long long) * 2 * MK_MAXBLOCKS,
                 MK_WS_BYTES = MK_WS_OFF + sizeof(long long) * 2 * MK_MAXBLOCKS;

// all pointers DEVICE; enqueues everything on stream
static hipError_t enqueue_mark(int64_t n, const double* eta2, double theta, int32_t* marked, int64_t* nmarked,
                               double* eta2_total, char* ws, hipStream_t stream)
{
  MarkState* st = reinterpret_cast<MarkState*>(ws);
  double* psum = reinterpret_cast<double*>(ws + MK_WS_PSUM);
  int* pcnt = reinterpret_cast<int*>(ws + MK_WS_PCNT);
  long long* bc = reinterpret_cast<long long*>(ws + MK_WS_BC);
  long long* off = reinterpret_cast<long long*>(ws + MK_WS_OFF);
  const int G = mark_blocks(n);
  const int all = std::fabs(theta - 1.0) <= 1e-8 ? 1 : 0; // np.isclose(doerfler, 1.0) of the reference
  hipError_t e = hipMemsetAsync(st, 0, sizeof(MarkState), stream);
  if (e != hipSuccess)
    return e;
  const int npass = all ? 1 : MK_PASSES; // all cells: the first pass for the total and the validity count only
  for (int p = 0; p < npass; ++p)
  {
    const int shift = 64 - MK_DIGIT_BITS * (p + 1);
    if (p == 0)
      hipLaunchKernelGGL(k_mark_histogram<true>, dim3(G), dim3(MK_THREADS), 0, stream, n, eta2, shift, st, psum, pcnt);
    else
      hipLaunchKernelGGL(k_mark_histogram<false>, dim3(G), dim3(MK_THREADS), 0, stream, n, eta2, shift, st, psum,
                         pcnt);
    hipLaunchKernelGGL(k_mark_select, dim3(1), dim3(MK_THREADS), 0, stream, n, G, p, theta, all, st, psum, pcnt);
  }
  hipLaunchKernelGGL(k_mark_count, dim3(G), dim3(MK_THREADS), 0, stream, n, eta2, st, bc);
  hipLaunchKernelGGL(k_mark_scan, dim3(1), dim3(MK_MAXBLOCKS), 0, stream, G, st, bc, off, nmarked, eta2_total);
  hipLaunchKernelGGL(k_mark_write, dim3(G), dim3(MK_THREADS), 0, stream, n, eta2, st, off, marked);
  return hipGetLastError();
}

static hipError_t enqueue_indicator(int64_t n, int nterms, int pair, const TermPtrs& tp, double* cell_eta2,
                                    double* totals, double* part, hipStream_t stream)
{
  const int G = mark_blocks(n);
  hipLaunchKernelGGL(k_indicator_total, dim3(G), dim3(MK_THREADS), 0, stream, n, nterms, pair, tp, cell_eta2,
                     totals ? part : nullptr);
  if (totals)
    hipLaunchKernelGGL(k_indicator_reduce, dim3(1), dim3(MK_THREADS), 0, stream, G, nterms, part, totals);
  return hipGetLastError();
}

} // namespace eqlb

extern "C" {

int eqlb_indicator_total(int64_t ncells, int32_t nterms, const double* const* terms, int32_t pair_last_two,
                         double* cell_eta2, double* totals, int32_t memspace, void* stream_)
{
  using namespace eqlb;
  if (ncells < 1 || nterms < 1 || nterms > MK_MAXTERMS || !terms || (pair_last_two && nterms < 2))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_indicator_total: invalid argument");
  for (int j = 0; j < nterms; ++j)
    if (!terms[j])
      return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_indicator_total: invalid argument");
  EQLB_TRY(check_memspace("eqlb_indicator_total", memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const size_t npart = (size_t)(MK_MAXTERMS + 1) * MK_MAXBLOCKS;
  const int pair = pair_last_two ? 1 : 0;
  TermPtrs tp = {};
  if (memspace == EQLB_MEM_DEVICE)
  {
    for (int j = 0; j < nterms; ++j)
      tp.p[j] = terms[j];
    StreamBuf part;
    if (totals && part.alloc(sizeof(double) * npart, stream) != hipSuccess)
      return fail(EQLB_ERR_DEVICE, "eqlb_indicator_total: device allocation failed");
    const hipError_t e = enqueue_indicator(ncells, nterms, pair, tp, cell_eta2, totals, part.as<double>(), stream);
    return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "eqlb_indicator_total: %s", hipGetErrorString(e));
  }
  // host memory: stage, run, return finished values
  HostCall s;
  const auto d_part = s.scratch<double>(npart);
  const auto d_tot = s.out(totals, (size_t)nterms + 1), d_cell = s.out(cell_eta2, (size_t)ncells);
  DevPiece<double> d_term[MK_MAXTERMS];
  for (int j = 0; j < nterms; ++j)
    d_term[j] = s.in(terms[j], (size_t)ncells);
  if (s.upload(stream) != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "eqlb_indicator_total: device allocation failed");
  for (int j = 0; j < nterms; ++j)
    tp.p[j] = d_term[j];
  s.note(enqueue_indicator(ncells, nterms, pair, tp, d_cell, d_tot, d_part, stream));
  const hipError_t e = s.finish(stream);
  return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "eqlb_indicator_total: %s", hipGetErrorString(e));
}

int eqlb_mark_doerfler(int64_t ncells, const double* cell_eta2, double theta, int32_t* marked, int64_t* nmarked,
                       double* eta2_total, int32_t memspace, void* stream_)
{
  using namespace eqlb;
  if (ncells < 1 || ncells > INT32_MAX || !cell_eta2 || !marked || !nmarked)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mark_doerfler: invalid argument (ncells = %lld)", (long long)ncells);
  if (!(theta > 0.0 && theta <= 1.0 + 1e-8))
    return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mark_doerfler: theta = %g outside (0, 1]", theta);
  EQLB_TRY(check_memspace("eqlb_mark_doerfler", memspace));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (memspace == EQLB_MEM_DEVICE)
  {
    StreamBuf ws;
    if (ws.alloc(MK_WS_BYTES, stream) != hipSuccess)
      return fail(EQLB_ERR_DEVICE, "eqlb_mark_doerfler: device allocation failed");
    const hipError_t e = enqueue_mark(ncells, cell_eta2, theta, marked, nmarked, eta2_total, ws.as<char>(), stream);
    return e == hipSuccess ? EQLB_OK : fail(EQLB_ERR_DEVICE, "eqlb_mark_doerfler: %s", hipGetErrorString(e));
  }
  for (int64_t i = 0; i < ncells; ++i)
    if (!(cell_eta2[i] >= 0.0))
      return fail(EQLB_ERR_INVALID_ARGUMENT, "eqlb_mark_doerfler: negative or NaN indicator in cell %lld",
                  (long long)i);
  // host memory: stage, run, return finished values; only marked[0 .. nmarked) is written
  int64_t nm = 0;
  double total = 0.0;
  HostCall s;
  const auto d_ws = s.scratch<char>(MK_WS_BYTES);
  const auto d_n = s.out(&nm, 1);
  const auto d_total = s.out(&total, 1);
  const auto d_eta = s.in(cell_eta2, (size_t)ncells);
  const auto d_marked = s.scratch<int32_t>((size_t)ncells);
  if (s.upload(stream) != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "eqlb_mark_doerfler: device allocation failed");
  s.note(enqueue_mark(ncells, d_eta, theta, d_marked, d_n, d_total, d_ws, stream));
  hipError_t e = s.finish(stream);
  if (e == hipSuccess && nm > 0 && nm <= ncells)
  {
    s.out_prefix(marked, d_marked, (size_t)nm);
    e = s.finish(stream);
  }
  if (e != hipSuccess)
    return fail(EQLB_ERR_DEVICE, "eqlb_mark_doerfler: %s", hipGetErrorString(e));
  if (nm < 1 || nm > ncells)
    return fail(EQLB_ERR_DEVICE, "eqlb_mark_doerfler: the device returned %lld marked cells", (long long)nm);
  *nmarked = nm;
  if (eta2_total)
    *eta2_total = total;
  return EQLB_OK;
}

} // extern "C"
