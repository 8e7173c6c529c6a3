// Greedy conditional-variance selection of inducing inputs ("choosing Z"): a pivoted partial Cholesky
// factorisation of Kff = K(X, X) that never forms Kff.  With d_i = sf2 at the start, step t picks the row j with the largest
// d (the lowest index among equals), forms the panel column
//       l_it = (k(x_i, x_j) - sum_{s < t} l_is l_js) / sqrt(d_j)        (s ascending)
// and lowers d_i by l_it^2 (clipped at 0; d_j = 0 exactly); sum_i d_i = tr(Kff - Qff) with Z = the rows picked so far.
//
//   select_init_kernel   x_id / ls_d transposed ([d][i]: coalesced over the rows), d = sf2, the first partials
//   select_step_kernel   ONE launch per pivot.  Every workgroup reduces the partials (largest d, its lowest index, sum of d)
//                        that the previous launch left, all in the same order: all reach the same pivot and the same stop
//                        decision, and the only hand-off between workgroups is the launch boundary - no tickets, flags, spins
//                        or fences, nothing that can hang.  Then it stages the pivot's coordinates and, in chunks of
//                        SEL_CHUNK doubles, the pivot's panel row in LDS, and for its own rows forms the dot product, the new
//                        column and the new d, and writes its partial.
//                        The closing launch (t == m_max, one workgroup) only records the last trace value.
//
// Panel layout: transposed, Lt[s][i] with leading dimension ldn = n rounded up to 32: the loads of step t are coalesced over
// the rows i, 16 bytes per lane (a lane owns two neighbouring rows).  The partials are kept twice and alternate with the
// parity of t: a workgroup may write its partial of step t while another one still reads those of step t - 1.  A launch that
// stops carries its own partial over to the other copy and writes nothing else, so every later launch sees the same partials
// and stops as well: neither a host round trip nor a device-side flag decides the stop.
// The kernel value is formed as cross_t_kernel (gpk_gram.hip) forms it: exact differences of the length-scale-divided
// coordinates, FMA accumulation, sf2 * gpk_exp_neg(-d2 / 2).  Every sum runs in an order fixed by (n, m_max); no atomics.
#include <cmath>

#include "gpk_internal.h"
#include "gpk_math.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_ROWS = 2 * SEL_THREADS;   // rows of one pass of a workgroup: two neighbouring rows per lane
constexpr int SEL_MAX_WGS = 2048;           // partials that every workgroup reduces per step
constexpr int SEL_CHUNK = 1024;             // doubles of the pivot's panel row staged in LDS at a time (8 KiB)
constexpr int SEL_MAX_D = 16;
constexpr int64_t SEL_MAX_M = 16384;

struct SelLs { double v[SEL_MAX_D]; };

// the work area: [Lt: m_max x ldn | Xs: 16 x ldn | d: ldn | partials: 2 x (max, sum: double; index: int64) x SEL_MAX_WGS]
struct SelPlan {
  int64_t ldn, rows_per_wg, nwg;
  int passes;
  size_t off_xs, off_d, off_pmax, off_psum, off_pidx, doubles;
};

SelPlan sel_plan(int64_t n, int64_t m_max) {
  SelPlan p;
  p.ldn = (n + 31) / 32 * 32;
  p.passes = (int)((n + (int64_t)SEL_ROWS * SEL_MAX_WGS - 1) / ((int64_t)SEL_ROWS * SEL_MAX_WGS));
  p.rows_per_wg = (int64_t)SEL_ROWS * p.passes;
  p.nwg = (n + p.rows_per_wg - 1) / p.rows_per_wg;
  p.off_xs = (size_t)m_max * p.ldn;
  p.off_d = p.off_xs + (size_t)SEL_MAX_D * p.ldn;
  p.off_pmax = p.off_d + (size_t)p.ldn;
  p.off_psum = p.off_pmax + 2 * SEL_MAX_WGS;
  p.off_pidx = p.off_psum + 2 * SEL_MAX_WGS;
  p.doubles = p.off_pidx + 2 * SEL_MAX_WGS;
  return p;
}

// (value descending, index ascending); a NaN never wins
__device__ __forceinline__ void sel_better(double& bv, long long& bi, double v, long long i) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// The workgroup's (largest value, its lowest index, sum) from one triple per thread: a tree over the threads in a fixed order.
// Every thread returns the result.
__device__ __forceinline__ void sel_block_reduce(double& bv, long long& bi, double& sum, double* sv, long long* si, double* ss) {
  const int tid = threadIdx.x;
  __syncthreads();      // (the arrays may still be read from the previous reduction)
  sv[tid] = bv; si[tid] = bi; ss[tid] = sum;
  __syncthreads();
  for (int off = SEL_THREADS / 2; off >= 1; off >>= 1) {
    if (tid < off) {
      double v = sv[tid];
      long long i = si[tid];
      sel_better(v, i, sv[tid + off], si[tid + off]);
      sv[tid] = v; si[tid] = i;
      ss[tid] += ss[tid + off];
    }
    __syncthreads();
  }
  bv = sv[0]; bi = si[0]; sum = ss[0];
}

__global__ __launch_bounds__(SEL_THREADS) void select_init_kernel(const double* __restrict__ X, long long n, int D, SelLs ls,
                                                                  double sf2, long long ldn, long long rows_per_wg,
                                                                  double* __restrict__ Xs, double* __restrict__ d,
                                                                  double* __restrict__ pmax, double* __restrict__ psum,
                                                                  long long* __restrict__ pidx, long long* __restrict__ selected) {
  __shared__ double sv[SEL_THREADS], ss[SEL_THREADS];
  __shared__ long long si[SEL_THREADS];
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * rows_per_wg;
  const long long r1 = min(r0 + rows_per_wg, ldn);
  double bv = -1.0, sum = 0.0;
  long long bi = r0;
  for (long long i = r0 + tid; i < r1; i += SEL_THREADS) {
    const bool in = i < n;
    for (int k = 0; k < D; ++k) Xs[k * ldn + i] = in ? X[i * D + k] / ls.v[k] : 0.0;
    const double di = in ? sf2 : 0.0;
    d[i] = di;
    if (in) sel_better(bv, bi, di, i);
    sum += di;
  }
  sel_block_reduce(bv, bi, sum, sv, si, ss);
  if (tid == 0) {
    pmax[blockIdx.x] = bv; psum[blockIdx.x] = sum; pidx[blockIdx.x] = bi;
    if (blockIdx.x == 0) selected[0] = 0;
  }
}

__global__ __launch_bounds__(SEL_THREADS) void select_step_kernel(long long n, int D, double sf2, long long ldn, long long rows_per_wg,
                                                                  int passes, int nwg, int t, int m_max, double var_stop,
                                                                  double sum_stop, const double* __restrict__ Xs,
                                                                  double* __restrict__ Lt, double* __restrict__ d,
                                                                  double* __restrict__ pmax, double* __restrict__ psum,
                                                                  long long* __restrict__ pidx, long long* __restrict__ idx,
                                                                  double* __restrict__ trace, double* __restrict__ dmax,
                                                                  long long* __restrict__ selected) {
  __shared__ double sv[SEL_THREADS], ss[SEL_THREADS];
  __shared__ long long si[SEL_THREADS];
  __shared__ __attribute__((aligned(16))) double prow[SEL_CHUNK];
  __shared__ double xj[SEL_MAX_D];
  const int tid = threadIdx.x;
  const int rd = (t & 1) * SEL_MAX_WGS, wr = ((t + 1) & 1) * SEL_MAX_WGS;

  // 1. the pivot and the stop decision from the previous launch's partials: the same order in every workgroup
  double bv = -1.0, sum = 0.0;
  long long bi = 0;
  for (int e = tid; e < nwg; e += SEL_THREADS) {
    sel_better(bv, bi, pmax[rd + e], pidx[rd + e]);
    sum += psum[rd + e];
  }
  sel_block_reduce(bv, bi, sum, sv, si, ss);
  const long long j = bi;
  const double dj = bv;
  if (blockIdx.x == 0 && tid == 0 && t >= 1 && selected[0] == t) trace[t - 1] = sum;    // step t - 1 was taken: its trace
  if (t == m_max) return;                                                               // the closing launch
  const bool stop = !(dj > var_stop) || (t >= 1 && sum <= sum_stop) || j < 0 || j >= n;
  if (stop) {      // the next launch reads the other copy: it must find these partials there
    if (tid == 0) { pmax[wr + blockIdx.x] = pmax[rd + blockIdx.x]; psum[wr + blockIdx.x] = psum[rd + blockIdx.x]; pidx[wr + blockIdx.x] = pidx[rd + blockIdx.x]; }
    return;
  }
  if (blockIdx.x == 0 && tid == 0) { idx[t] = j; dmax[t] = dj; selected[0] = t + 1; }
  const double rs = __builtin_sqrt(dj);

  // 2. the pivot's scaled coordinates
  if (tid < D) xj[tid] = Xs[tid * ldn + j];

  // 3. the rows of this workgroup, SEL_ROWS per pass, two neighbouring rows per lane
  const long long r0 = (long long)blockIdx.x * rows_per_wg;
  bv = -1.0; sum = 0.0; bi = r0;
  for (int ps = 0; ps < passes; ++ps) {
    const long long i = r0 + (long long)ps * SEL_ROWS + 2 * tid;      // even; i + 1 < ldn whenever i < ldn
    const bool live = i < n;      // (wave-uniform except in the last wave with rows)
    double a0 = 0.0, a1 = 0.0;
    for (int s0 = 0; s0 < t; s0 += SEL_CHUNK) {
      const int sc = min(SEL_CHUNK, t - s0);
      __syncthreads();      // prow may still be read (previous chunk / pass); xj is written
      for (int e = tid; e < sc; e += SEL_THREADS) prow[e] = Lt[(size_t)(s0 + e) * ldn + j];
      __syncthreads();
      if (live) {
        const double* col = Lt + (size_t)s0 * ldn + i;
#pragma unroll 8
        for (int s = 0; s < sc; ++s) {
          const double2 v = *reinterpret_cast<const double2*>(col + (size_t)s * ldn);
          const double p = prow[s];
          a0 = __builtin_fma(v.x, p, a0);
          a1 = __builtin_fma(v.y, p, a1);
        }
      }
    }
    if (t == 0) __syncthreads();      // xj
    if (live) {
      double q0 = 0.0, q1 = 0.0;
      for (int k = 0; k < D; ++k) {
        const double2 x = *reinterpret_cast<const double2*>(Xs + (size_t)k * ldn + i);
        const double e0 = x.x - xj[k], e1 = x.y - xj[k];
        q0 = __builtin_fma(e0, e0, q0);
        q1 = __builtin_fma(e1, e1, q1);
      }
      const double2 dd = *reinterpret_cast<const double2*>(d + i);
      const double l0 = (sf2 * gpk_exp_neg(-0.5 * q0) - a0) / rs;
      const double l1 = (sf2 * gpk_exp_neg(-0.5 * q1) - a1) / rs;
      double d0 = fmax(dd.x - l0 * l0, 0.0), d1 = fmax(dd.y - l1 * l1, 0.0);
      const bool in1 = i + 1 < n;
      if (i == j) d0 = 0.0;
      if (i + 1 == j || !in1) d1 = 0.0;
      double2 lo; lo.x = l0; lo.y = in1 ? l1 : 0.0;
      double2 dn; dn.x = d0; dn.y = d1;
      *reinterpret_cast<double2*>(Lt + (size_t)t * ldn + i) = lo;
      *reinterpret_cast<double2*>(d + i) = dn;
      sel_better(bv, bi, d0, i);
      if (in1) sel_better(bv, bi, d1, i + 1);
      sum += d0;
      sum += d1;
    }
  }

  // 4. this workgroup's partial
  sel_block_reduce(bv, bi, sum, sv, si, ss);
  if (tid == 0) { pmax[wr + blockIdx.x] = bv; psum[wr + blockIdx.x] = sum; pidx[wr + blockIdx.x] = bi; }
}

}  // namespace

extern "C" size_t gpk_greedy_select_bytes(int64_t n, int64_t m_max) {
  if (n < 1 || m_max < 1 || m_max > SEL_MAX_M || n >= (1ll << 40)) return 0;
  return sel_plan(n, m_max).doubles * sizeof(double);
}

extern "C" int gpk_greedy_select(gpk_handle h, const double* X, int64_t n, int D, const double* ls, int n_ls, double sf2,
                                 int64_t m_max, double min_var, double tol, void* work, int64_t* idx, double* trace, double* dmax,
                                 int64_t* selected) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && ls && work && idx && trace && dmax && selected, "greedy_select: null pointer");
  GPK_REQUIRE(h, n >= 1 && n < (1ll << 40), "greedy_select: need 1 <= n < 2^40 rows");
  GPK_REQUIRE(h, m_max >= 1 && m_max <= n && m_max <= SEL_MAX_M, "greedy_select: need 1 <= m_max <= min(n, 16384)");
  GPK_REQUIRE(h, D >= 1 && D <= SEL_MAX_D, "greedy_select: need 1 <= D <= 16");
  GPK_REQUIRE(h, n_ls == 1 || n_ls == D, "greedy_select: n_ls must be 1 (isotropic) or D (ARD)");
  GPK_REQUIRE(h, sf2 > 0.0 && std::isfinite(sf2), "greedy_select: sf2 must be positive");
  GPK_REQUIRE(h, min_var >= 0.0 && tol >= 0.0 && std::isfinite(min_var) && std::isfinite(tol),
              "greedy_select: min_var and tol must be non-negative");
  GPK_REQUIRE(h, ((uintptr_t)work % 16) == 0, "greedy_select: the work area must be 16-byte aligned");
  GPK_REQUIRE(h, h->batch == 1, "greedy_select: not available in batched mode");
  SelLs l;
  for (int k = 0; k < SEL_MAX_D; ++k) l.v[k] = 1.0;
  for (int k = 0; k < D; ++k) {
    l.v[k] = ls[n_ls == 1 ? 0 : k];
    GPK_REQUIRE(h, l.v[k] > 0.0 && std::isfinite(l.v[k]), "greedy_select: length-scales must be positive");
  }
  const SelPlan p = sel_plan(n, m_max);
  double* w = (double*)work;
  double* Lt = w;
  double* Xs = w + p.off_xs;
  double* d = w + p.off_d;
  double* pmax = w + p.off_pmax;
  double* psum = w + p.off_psum;
  long long* pidx = (long long*)(w + p.off_pidx);
  const double var_stop = min_var * sf2, sum_stop = tol * (double)n * sf2;
  hipLaunchKernelGGL(select_init_kernel, dim3((unsigned)p.nwg), dim3(SEL_THREADS), 0, h->stream, X, (long long)n, D, l, sf2,
                     (long long)p.ldn, (long long)p.rows_per_wg, Xs, d, pmax, psum, pidx, (long long*)selected);
  GPK_LAUNCH_CHECK(h);
  for (int t = 0; t <= (int)m_max; ++t) {      // t == m_max: the closing launch, one workgroup
    hipLaunchKernelGGL(select_step_kernel, dim3(t == (int)m_max ? 1u : (unsigned)p.nwg), dim3(SEL_THREADS), 0, h->stream,
                       (long long)n, D, sf2, (long long)p.ldn, (long long)p.rows_per_wg, p.passes, (int)p.nwg, t, (int)m_max,
                       var_stop, sum_stop, Xs, Lt, d, pmax, psum, pidx, (long long*)idx, trace, dmax, (long long*)selected);
    GPK_LAUNCH_CHECK(h);
  }
  return GPK_OK;
}
