// Small-batch serving kernels (fp64; M <= 32 queries, D <= 16, P <= 16, Np <= 16384): the control loop's
// single-row `predict_residual` and horizon-25 calls (simple_gp.py:175-206, gaussian_process.py:199-240).
// The general chain spends seven launches (copy, fused mean, mean reduce, K*^T, tile GEMM on a 128-query
// panel, column-sum reduce, finalize = 80 us of GPU time for 25 queries at N = 1000); here it is two:
//
//   small_cross_mean_kernel  32 training rows per workgroup: K*[m][j] = sf2 exp(-|x_j - q_m|^2 / 2) (exact
//                            differences of inputs divided by the length-scale, as everywhere else), written
//                            query-major for the second kernel, and the workgroup's share of K* alpha; the last
//                            workgroup to finish adds the shares in a fixed order and writes the means.
//   small_var_kernel         16 rows of W = L^-1 per workgroup: V = W K*^T as a 16 x (16|32) x k product on
//                            v_mfma_f64_16x16x4_f64 (both operands read straight from L2: each lane's
//                            16-byte pieces are k-contiguous), the k-range split over the 4 waves; squares
//                            summed over the rows; the last workgroup adds the shares and writes
//                            max(kss - sum, floor).
//   small_cov_kernel         the same rows of V = W K*^T per workgroup; instead of squares it stores the workgroup's
//                            share V_r^T V_r (lower triangle of the 32 x 32 block); the shares are added in a fixed
//                            order in two levels - the last workgroup of each group of CG adds its group's, the last
//                            of those adds the group sums - and K(Xq, Xq) + noise I - sum is written, mirrored.
//                            The model is blockIdx.y as in the other two: the per-axis batch gets the B joint covariances
//                            in the same two launches, each model with its own shares, group sums and ticket counters.
//
//   input gradients (K8)     small_cross_mean_jac_kernel adds the workgroup's share of the mean Jacobian
//                            sum_j k*_mj alpha_jp (x_jd - q_md) / ls_d to the same launch (mean + Jacobian: still ONE launch,
//                            the last workgroup adds both kinds of shares in a fixed order); for the variance gradient
//                            small_var_grad_kernel also stores its rows of V = W K*^T, and small_wtv_grad_kernel - 16
//                            columns of W per workgroup - forms C = W^T V, its share of sum_j k*_mj C_jm (x_jd - q_md) / ls_d
//                            and, in the last workgroup, -2 / ls_d times the fixed-order sum of the shares.
//                            All three take the model as a grid dimension (blockIdx.y, y, z) like the mean and the variance:
//                            the per-axis batch (B <= 8 single-output models on one query batch) gets mean + Jacobian of
//                            every model in ONE launch and all four results in three, each model
//                            with its own shares and its own ticket counters.
//
//   second derivatives (K8)  mean + Jacobian + the mean's input Hessian: small_cross_mean_jac_kernel, then small_hess_kernel (below,
//                            with its own description): two launches for any number of models and outputs.
//
//   a propagation stage (K11) mean + Jacobian + variance without the variance gradient: small_cross_mean_jac_kernel, then
//                            small_var_jac_kernel - small_var_grad_kernel's body without its store of V - and no W^T V launch: two
//                            launches with the bits of the three-launch call (gpk_propagate.hip chains them along a horizon, the
//                            queries in a device buffer).  small_var_jac2_kernel is its two-factor form (below: TWO), the sparse
//                            models' stage: var_out M x P (B x M for a batch), final.
//
//   ... at second order      one more launch per stage, small_hess_trace_kernel (below, with its own description): the workgroups' shares
//                            of tr(H Sigma) for every (query, output), R x NO scalars instead of R x NO x D x D Hessian entries;
//                            the chain's advance launch adds them.  gpk_small_trace_launch makes it.
//
//   ... in a backward stage   the gradient of a horizon cost (K11) needs H w for one vector w per (query, output): small_hvp_kernel (below,
//                            with its own description) - the workgroups' shares of the D + 1 sums per (query, output), the Hessian never
//                            formed; the chain's adjoint launch adds them.  gpk_small_hvp_launch makes it.
//
//   two factors (K9)         the sparse model's variance terms are kss - |Wuu k*|^2 + |WSigma k*|^2 on ONE K* with P outputs: the
//                            first launch runs with one model, and small_var[_grad]_kernel, small_cov_kernel and small_wtv_grad_kernel
//                            with the template parameter TWO - the same bodies - take the inverse FACTOR as the grid
//                            dimension that is the model elsewhere: shared K*, mean and Jacobian shares, per-factor V and shares, one
//                            ticket count over the workgroups of both, and the last workgroup overall writes the combination:
//                            any P at the launch counts of one model.
//   ... with a model dimension  the same kernels serve B <= 8 sparse models (P = 1 each, equal m and D, each with its own Z, alpha_u,
//                            kernel, noise, normalisation and factor pair) on one query batch: that grid dimension is 2 * model +
//                            factor.  Per model one K* and one set of mean / Jacobian shares (the cross kernels' blockIdx.y), per
//                            (model, factor) its own V and shares, per model ONE ticket count over the workgroups of both of its
//                            factors, and that model's last workgroup writes its combination.  A model's sums are grouped by (Np, M)
//                            alone: its block has the bits of that model served alone.
//
// The results land in the caller's (pinned, mapped) output block; the queries are read from it as well.  ONE host routine,
// gpk_small_launch, makes the launches of every call (predict, gradients, covariance) for B models of one or two inverse factors
// from a ServeModels (gpk_internal.h): its checks, the parameter block, the work area's pointers (small_work) and the grids.
#include "gpk_internal.h"
#include "gpk_math.h"

namespace {

constexpr int SQ = GPK_SMALL_MAX_M, SJ = 32, SD = 16, SP = 16, SR = 16;
struct Arr16 { double v[16]; };
constexpr size_t SMALLK_ARG_LIMIT = 2048;    // (kernel arguments: 4 KiB in all; the parameter block goes by value)
// Per-model parameters (model = blockIdx.y).  One model with P <= 16 outputs, or B <= 8 single-output models that
// share the query batch (the per-axis GPs of gp_trainer.py): output o = model * P + p indexes ymean / ystd.
struct SmallK {
  const double* X[GPK_SMALL_MAX_MODELS];
  const double* alpha[GPK_SMALL_MAX_MODELS];
  const double* W[GPK_SMALL_MAX_MODELS];
  const double* W2[GPK_SMALL_MAX_MODELS];   // the second inverse factor of a model (the two-factor kernels only)
  double ls[GPK_SMALL_MAX_MODELS][16];
  double sf2[GPK_SMALL_MAX_MODELS], kss[GPK_SMALL_MAX_MODELS];
  double ymean[16], ystd[16];
  double noise[GPK_SMALL_MAX_MODELS];   // the WhiteKernel level (covariance only)
};
static_assert(sizeof(SmallK) <= SMALLK_ARG_LIMIT, "the parameter block is a kernel argument");
typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2v __attribute__((ext_vector_type(2)));

// Every one of `count` workgroups has stored its share; true (in all its threads) for the last one to get here.  The
// barrier orders the workgroup's stores before thread 0's ticket; the ticket is one acquire-release atomic at device
// scope (release: the shares are written back before it; acquire: the last workgroup drops its cached lines before it
// reads the others' shares) -- one cache write-back per workgroup instead of one per wave.  The counter is left at
// zero for the next launch.
__device__ __forceinline__ bool last_of(unsigned* counter, unsigned count, int tid) {
  __shared__ int is_last;
  __syncthreads();
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    is_last = (t == count - 1);
    if (is_last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return is_last != 0;
}

// Sum of `count` shares p[(first + k * step) * stride], k = 0.., in that order; the loads go out eight at a time
// (the last workgroup reads them from memory: one dependent load per share would cost a miss latency each).
__device__ __forceinline__ double sum_shares(const double* p, unsigned first, unsigned step, unsigned shares,
                                             long long stride) {
  double s = 0.0;
  for (unsigned g = first; g < shares; g += 8 * step) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned gu = g + u * step;
      v[u] = p[(long long)min(gu, shares - 1) * stride];
      if (gu >= shares) v[u] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  return s;
}

// sum_shares for two share blocks at once (the two-factor kernels): both blocks' loads of a round go out together - the last
// workgroup waits for one miss latency per round, not two - and each block's shares are added in sum_shares' order.
__device__ __forceinline__ void sum_shares2(const double* p0, const double* p1, unsigned first, unsigned step, unsigned shares,
                                            long long stride, double& s0, double& s1) {
  s0 = 0.0;
  s1 = 0.0;
  for (unsigned g = first; g < shares; g += 8 * step) {
    double v0[8], v1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned gu = g + u * step;
      const long long at = (long long)min(gu, shares - 1) * stride;
      v0[u] = p0[at];
      v1[u] = p1[at];
      if (gu >= shares) { v0[u] = 0.0; v1[u] = 0.0; }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s0 += v0[u];
#pragma unroll
    for (int u = 0; u < 8; ++u) s1 += v1[u];
  }
}

// The fixed-order sum of the mean shares, by whichever workgroup finishes last.  `lds`: 4 * SQ * SP doubles.  The
// grouping of the sum depends on M * P only (256 threads take part whatever the workgroup size), so a mean-only
// call and a mean + variance call return the same bits.
__device__ __forceinline__ void finish_means(const double* pmean, unsigned shares, int M, int P, const double* ymean,
                                             const double* ystd, double* mean_out, int tid, double* lds) {
  constexpr int NT = 256;
  const int MP = M * P;
  const int nparts = 4 * MP <= NT ? 4 : (2 * MP <= NT ? 2 : 1);
  const int chunk = NT / nparts, part = tid / chunk, tl = tid - part * chunk;
  for (int base = 0; base < MP; base += chunk) {
    const int t = base + tl;
    if (tid < NT && t < MP) lds[part * (SQ * SP) + t] = sum_shares(pmean + t, part, nparts, shares, SQ * SP);
    __syncthreads();
    if (part == 0 && t < MP) {
      double s = lds[t];
      for (int k = 1; k < nparts; ++k) s += lds[k * (SQ * SP) + t];
      const int p = t % P;
      mean_out[t] = ymean[p] + ystd[p] * s;
    }
    if (base + chunk < MP) __syncthreads();      // another pass reuses the scratch
  }
}

// The fixed-order sum of the mean-Jacobian shares (pjac: shares x M * P * D, entry t = (m * P + p) * D + d), by one workgroup
// once every share is complete: dmean[m][p][d] = y_std[p] / ls_d * sum.
__device__ __forceinline__ void finish_jac(const double* pjac, unsigned shares, int M, int P, int D, const double* ystd,
                                           const double* ls, double* dmean_out, int tid, int nthreads) {
  const int MPD = M * P * D;
  // four entries per thread and eight shares of each in flight (the workgroup reads the shares from memory: with one entry
  // at a time the miss latencies of M P D / nthreads entries would queue up behind each other); every entry's shares are
  // added in share order whatever the grouping
  for (int base = 0; base < MPD; base += 4 * nthreads) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (unsigned g = 0; g < shares; g += 8) {
      double v[4][8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = min(base + tid + e * nthreads, MPD - 1);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          v[e][u] = pjac[(long long)min(g + u, shares - 1) * MPD + t];
          if (g + u >= shares) v[e][u] = 0.0;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int u = 0; u < 8; ++u) s[e] += v[e][u];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int t = base + tid + e * nthreads;
      if (t < MPD) dmean_out[t] = ystd[(t / D) % P] / ls[t % D] * s[e];
    }
  }
}

// FINISH: this launch is the only one (mean-only call) and elects the workgroup that writes the means; otherwise
// small_var_kernel's last workgroup does it.
// JAC (small_cross_mean_jac_kernel; model = blockIdx.y as for the mean): the launch also forms the mean Jacobian's shares (pjac) and - FINISH - the
// Jacobian itself (dmean_out).  The body is shared; small_cross_mean_kernel keeps its signature and its launches.
template <bool FINISH, bool JAC>
__device__ __forceinline__ void small_cross_mean_body(SmallK k, long long N, long long Np, int D, int P,
                                                               const double* __restrict__ Xq, int M, double* Ks,
                                                               double* pmean, unsigned* counter, double* mean_out,
                                                               double* pjac, double* dmean_out) {
  __shared__ double q[SQ][SD + 1];
  __shared__ double ks[SQ][SJ + 1];
  __shared__ double al[SJ][SP + 1];
  const int b = blockIdx.y;
  const double* __restrict__ X = k.X[b];
  const double* __restrict__ alpha = k.alpha[b];
  const double* ls = k.ls[b];
  const double sf2 = k.sf2[b];
  if (Ks) Ks += (long long)b * SQ * Np;
  pmean += (long long)b * gridDim.x * (SQ * SP);
  mean_out += (long long)b * M * P;
  counter += b;
  if constexpr (JAC) {
    pjac += (long long)b * gridDim.x * (M * P * D);
    dmean_out += (long long)b * M * P * D;
  }
  const int tid = threadIdx.x, jl = tid & 31, mg = tid >> 5;
  const long long j0 = (long long)blockIdx.x * SJ, j = j0 + jl;
  const bool valid = j < N;
  // all global reads first (the queries may sit in host memory: the longest latency), then their uses
  double qv[2], av[2], xr[SD];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = tid + 256 * u;
    qv[u] = (e < M * D) ? Xq[e] : 0.0;
    const int jj = e / P;
    av[u] = (e < SJ * P && j0 + jj < N) ? alpha[j0 * P + e] : 0.0;
  }
#pragma unroll
  for (int d = 0; d < SD; ++d) xr[d] = (d < D && valid) ? X[j * D + d] : 0.0;
#pragma unroll
  for (int d = 0; d < SD; ++d) xr[d] = xr[d] / ls[d];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = tid + 256 * u;
    if (e < SJ * P) al[e / P][e % P] = av[u];
    if (e < M * D) q[e / D][e % D] = qv[u] / ls[e % D];
  }
  __syncthreads();
#pragma unroll
  for (int mi = 0; mi < SQ / 8; ++mi) {
    const int m = mg + 8 * mi;
    if (m < M) {
      double d2 = 0.0;
#pragma unroll
      for (int d = 0; d < SD; ++d)
        if (d < D) {
          const double df = q[m][d] - xr[d];
          d2 = __builtin_fma(df, df, d2);
        }
      const double v = valid ? sf2 * gpk_exp_neg(-0.5 * d2) : 0.0;
      ks[m][jl] = v;
      if (Ks) Ks[(long long)m * Np + j] = v;
    }
  }
  double (*xs)[SD + 1] = nullptr;                   // JAC: the staged training rows, divided by the length-scales
  if constexpr (JAC) {
    __shared__ double xs_s[SJ][SD + 1];
    xs = xs_s;
    if (mg == 0) {
#pragma unroll
      for (int d = 0; d < SD; ++d) xs[jl][d] = xr[d];
    }
  }
  __syncthreads();
  for (int t = tid; t < M * P; t += 256) {
    const int m = t / P, p = t - m * P;
    double s = 0.0;
#pragma unroll 8
    for (int jj = 0; jj < SJ; ++jj) s = __builtin_fma(ks[m][jj], al[jj][p], s);
    pmean[(long long)blockIdx.x * (SQ * SP) + t] = s;
  }
  if constexpr (JAC) {
    // share of sum_j k*_mj alpha_jp (x_jd - q_md) / ls_d, entry t = (m * P + p) * D + d
    const int MPD = M * P * D;
    for (int t = tid; t < MPD; t += 256) {
      const int d = t % D, mp = t / D, p = mp % P, m = mp / P;
      const double qd = q[m][d];
      double s = 0.0;
#pragma unroll 8
      for (int jj = 0; jj < SJ; ++jj) s = __builtin_fma(ks[m][jj] * al[jj][p], xs[jj][d] - qd, s);
      pjac[(long long)blockIdx.x * MPD + t] = s;
    }
  }
  if constexpr (FINISH) {
    if (last_of(counter, gridDim.x, tid)) {
      __shared__ double fin[4 * SQ * SP];
      finish_means(pmean, gridDim.x, M, P, k.ymean + b * P, k.ystd + b * P, mean_out, tid, fin);
      if constexpr (JAC) finish_jac(pjac, gridDim.x, M, P, D, k.ystd + b * P, ls, dmean_out, tid, 256);
    }
  }
}

template <bool FINISH>
__global__ __launch_bounds__(256) void small_cross_mean_kernel(SmallK k, long long N, long long Np, int D, int P,
                                                               const double* __restrict__ Xq, int M, double* Ks,
                                                               double* pmean, unsigned* counter, double* mean_out) {
  small_cross_mean_body<FINISH, false>(k, N, Np, D, P, Xq, M, Ks, pmean, counter, mean_out, nullptr, nullptr);
}
template <bool FINISH>
__global__ __launch_bounds__(256) void small_cross_mean_jac_kernel(SmallK k, long long N, long long Np, int D, int P,
                                                                   const double* __restrict__ Xq, int M, double* Ks,
                                                                   double* pmean, unsigned* counter, double* mean_out,
                                                                   double* pjac, double* dmean_out) {
  small_cross_mean_body<FINISH, true>(k, N, Np, D, P, Xq, M, Ks, pmean, counter, mean_out, pjac, dmean_out);
}

// ---- the mean's input Hessian (K8, second derivatives): the second launch of a GPK_SMALL_HESS call ------------------------------
// With delta_mj = q_m - r_j (queries and rows divided by the length-scales, exact differences) and k*_mj as above:
//   T[m][p][d][e] = sum_j k*_mj alpha_jp delta_mjd delta_mje  (e <= d),   S[m][p] = sum_j k*_mj alpha_jp
//   hess[m][p][d][e] = hess[m][p][e][d] = y_std[p] / (ls_d ls_e) (T - [d = e] S)
// A workgroup takes hess_rows(Np) = max(32, Np / 64) training rows - at most 64 workgroups per model, so that the last one reads
// at most 64 shares - in rounds of HJ rows staged through LDS (K* recomputed: the first launch stores none without a variance).
// Its share is M * P * (D (D + 1) / 2 + 1) doubles, entry t = (m * P + p) * TP + (packed (d, e), or TP - 1 for S); every entry is
// owned by one thread, which carries it from round to round through the share itself.  The (query, output) pairs are cut into
// slices of hess_slice(D) pairs - about 512 entries - over the third grid dimension: a workgroup forms its slice of its rows'
// share, and the last workgroup OF A SLICE (last_of on the counter of (model, slice), left at zero) adds that slice of the
// shares in workgroup order, one thread per (m, p, d, e <= d), and writes both triangles from the one sum - the final sums of a
// call (2 MB of shares at M = 25, P = 6, D = 10, Np = 1024) are spread over as many workgroups as there are slices instead of
// queueing in one.  Rows, slices and the order of every sum depend on (Np, M, P, D) alone: block b of a batch has the bits of
// model b alone.
constexpr int HJ = 32;
constexpr int HT_MAX = SD * (SD + 1) / 2;      // 136 packed triangle entries at D = 16
constexpr int HESS_SLICE_ENTRIES = 512;
__host__ __device__ inline long long hess_rows(long long Np) { return Np / 64 < 32 ? 32 : Np / 64; }
// (query, output) pairs per slice: whole pairs, so that a slice holds the S of its own diagonals
__host__ __device__ inline int hess_slice(int D) { const int n = HESS_SLICE_ENTRIES / (D * (D + 1) / 2 + 1); return n < 1 ? 1 : n; }

__global__ __launch_bounds__(256) void small_hess_kernel(SmallK k, long long N, long long Np, int D, int P,
                                                         const double* __restrict__ Xq, int M, double* phess, unsigned* counter,
                                                         double* hess_out) {
  __shared__ double q[SQ][SD + 1];
  __shared__ double ks[SQ][HJ + 1];
  __shared__ double al[HJ][SP + 1];
  __shared__ double xs[HJ][SD + 1];
  __shared__ unsigned char td[HT_MAX + 1], te[HT_MAX + 1];
  const int b = blockIdx.y, tid = threadIdx.x;
  const double* __restrict__ X = k.X[b];
  const double* __restrict__ alpha = k.alpha[b];
  const double* ls = k.ls[b];
  const double sf2 = k.sf2[b];
  const int TT = D * (D + 1) / 2, TP = TT + 1, E = M * P * TP;
  const long long rows = hess_rows(Np);
  const long long r0 = (long long)blockIdx.x * rows, r1 = min(N, r0 + rows);
  double* share = phess + ((long long)b * gridDim.x + blockIdx.x) * E;
  const int mps = hess_slice(D), mp0 = blockIdx.z * mps, mp1 = min(M * P, mp0 + mps);      // this slice's pairs (mp0 < M P)
  const int m_lo = mp0 / P, m_hi = (mp1 - 1) / P, t0 = mp0 * TP, t1 = mp1 * TP;
  for (int t = tid; t < TT; t += 256) {
    int d = 0;
    while ((d + 1) * (d + 2) / 2 <= t) ++d;
    td[t] = (unsigned char)d;
    te[t] = (unsigned char)(t - d * (d + 1) / 2);
  }
  for (int e = tid; e < M * D; e += 256) q[e / D][e % D] = Xq[e] / ls[e % D];
  // (a workgroup past the last training row runs one empty round: its share is zeros and its ticket is taken)
  for (long long jb = r0; jb < r1 || jb == r0; jb += HJ) {
    __syncthreads();
    for (int e = tid; e < HJ * D; e += 256) {
      const int jj = e / D, d = e - jj * D;
      xs[jj][d] = (jb + jj < r1) ? X[(jb + jj) * D + d] / ls[d] : 0.0;
    }
    for (int e = tid; e < HJ * P; e += 256) {
      const int jj = e / P, p = e - jj * P;
      al[jj][p] = (jb + jj < r1) ? alpha[(jb + jj) * P + p] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < (m_hi - m_lo + 1) * HJ; e += 256) {
      const int m = m_lo + e / HJ, jj = e % HJ;
      double d2 = 0.0;
      for (int d = 0; d < D; ++d) {
        const double df = q[m][d] - xs[jj][d];
        d2 = __builtin_fma(df, df, d2);
      }
      ks[m][jj] = (jb + jj < r1) ? sf2 * gpk_exp_neg(-0.5 * d2) : 0.0;
    }
    __syncthreads();
    for (int t = t0 + tid; t < t1; t += 256) {
      const int mp = t / TP, tt = t - mp * TP, m = mp / P, p = mp - m * P;
      double s = (jb == r0) ? 0.0 : share[t];
      if (tt == TT) {
#pragma unroll 8
        for (int jj = 0; jj < HJ; ++jj) s = __builtin_fma(ks[m][jj], al[jj][p], s);
      } else {
        const int d = td[tt], e = te[tt];
        const double qd = q[m][d], qe = q[m][e];
#pragma unroll 8
        for (int jj = 0; jj < HJ; ++jj) s = __builtin_fma(ks[m][jj] * al[jj][p] * (qd - xs[jj][d]), qe - xs[jj][e], s);
      }
      share[t] = s;
    }
  }
  if (last_of(counter + b * gridDim.z + blockIdx.z, gridDim.x, tid)) {
    const double* base = phess + (long long)b * gridDim.x * E;
    const double* ystd = k.ystd + b * P;
    double* out = hess_out + (long long)b * M * P * D * D;
    for (int t = mp0 * TT + tid; t < mp1 * TT; t += 256) {
      const int mp = t / TT, tt = t - mp * TT, p = mp % P, d = td[tt], e = te[tt];
      double s = sum_shares(base + (long long)mp * TP + tt, 0, 1, gridDim.x, E);
      if (d == e) s -= sum_shares(base + (long long)mp * TP + TT, 0, 1, gridDim.x, E);
      const double v = ystd[p] / (ls[d] * ls[e]) * s;
      out[((long long)mp * D + d) * D + e] = v;
      out[((long long)mp * D + e) * D + d] = v;
    }
  }
}

// ---- tr(H Sigma) of the mean's input Hessian (K11, second order): the third launch of a second-order propagation stage ------------
// The contraction of small_hess_kernel's result with a covariance, formed without the Hessian.  Query m carries its own nx x nx
// covariance Sg[m] (raw units, the chain's state).  With delta_mj = q_m - r_j as above (d < nx only: the controls are exact) and
//   St[m][d][e] = Sg[m][d][e] / (in_scale_d ls_d in_scale_e ls_e)       (this model's own length-scales),
//   tr(H_mp Sg_m) = y_std[p] (T[m][p] - tr St[m] S[m][p]),   T[m][p] = sum_j k*_mj alpha_jp delta_mj^T St[m] delta_mj,
//                                                            S[m][p] = sum_j k*_mj alpha_jp
// The workgroups take small_hess_kernel's rows (hess_rows(Np), at most 64 workgroups per model) in its rounds of HJ rows, K*
// recomputed from the device query rows.  Per (query, row) ONE quadratic form over the packed triangle of St (off-diagonal
// entries stored doubled), per (query, output) two fixed-order sums carried in registers from round to round; the workgroup
// writes them to its own slot, shares[(group * E + e) * 2 + {0: T, 1: S}] with e = (model * M + m) * P + p and E = B M P, and
// workgroup 0 of a model writes tr St[m] to trs[model * M + m].  No ticket and no last workgroup: the chain's advance launch
// adds the slots in workgroup order.  Rows past N enter as zeros, a workgroup past the last row writes zeros, every slot is
// written, and rows, rounds and the order of every sum depend on (Np, M, P, D, nx) alone: model b of a batch has the bits of
// model b alone.
constexpr int TRACE_PAIRS = SQ * HJ / 256;       // (query, row) pairs per thread and round
constexpr int TRACE_OUTS = SQ * SP / 256;        // (query, output) sums per thread

__global__ __launch_bounds__(256) void small_hess_trace_kernel(SmallK k, Arr16 in_scale, long long N, long long Np, int D, int P, int nx,
                                                               const double* __restrict__ Xq, const double* __restrict__ Sg, int M,
                                                               double* shares, double* trs) {
  __shared__ double q[SQ][SD + 1];
  __shared__ double ks[SQ][HJ + 1];
  __shared__ double kq[SQ][HJ + 1];
  __shared__ double al[HJ][SP + 1];
  __shared__ double xs[HJ][SD + 1];
  __shared__ double St[SQ][HT_MAX];
  __shared__ double ls[SD], sl[SD];      // the model's length-scales; in_scale * ls
  const int b = blockIdx.y, tid = threadIdx.x;
  const double* __restrict__ X = k.X[b];
  const double* __restrict__ alpha = k.alpha[b];
  const double sf2 = k.sf2[b];
  const int TT = nx * (nx + 1) / 2, MP = M * P;
  const long long rows = hess_rows(Np);
  const long long r0 = (long long)blockIdx.x * rows, r1 = min(N, r0 + rows);
  if (tid < SD) {
    ls[tid] = k.ls[b][tid];
    sl[tid] = in_scale.v[tid] * k.ls[b][tid];
  }
  __syncthreads();
  // (queries and rows are staged to the full width SD, zeros from D on: the differences below take no select)
  for (int e = tid; e < M * SD; e += 256) {
    const int m = e / SD, d = e % SD;
    q[m][d] = d < D ? Xq[m * D + d] / ls[d] : 0.0;
  }
  for (int t = tid; t < M * TT; t += 256) {
    const int m = t / TT, tt = t - m * TT;
    int d = 0;
    while ((d + 1) * (d + 2) / 2 <= tt) ++d;
    const int e = tt - d * (d + 1) / 2;
    const double s = Sg[((long long)m * nx + d) * nx + e] / (sl[d] * sl[e]);
    St[m][tt] = d == e ? s : 2.0 * s;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < M) {
    double t = 0.0;
    for (int d = 0; d < nx; ++d) t += St[tid][d * (d + 1) / 2 + d];
    trs[b * M + tid] = t;
  }
  double accT[TRACE_OUTS], accS[TRACE_OUTS];
#pragma unroll
  for (int u = 0; u < TRACE_OUTS; ++u) accT[u] = accS[u] = 0.0;
  for (long long jb = r0; jb < r1; jb += HJ) {
    __syncthreads();
    for (int e = tid; e < HJ * SD; e += 256) {
      const int jj = e / SD, d = e % SD;
      xs[jj][d] = (d < D && jb + jj < r1) ? X[(jb + jj) * D + d] / ls[d] : 0.0;
    }
    for (int e = tid; e < HJ * P; e += 256) {
      const int jj = e / P, p = e - jj * P;
      al[jj][p] = (jb + jj < r1) ? alpha[(jb + jj) * P + p] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TRACE_PAIRS; ++u) {
      const int e = tid + 256 * u, m = e / HJ, jj = e % HJ;
      if (m < M) {
        double dl[SD], d2 = 0.0;
#pragma unroll
        for (int d = 0; d < SD; ++d) {
          dl[d] = q[m][d] - xs[jj][d];
          d2 = __builtin_fma(dl[d], dl[d], d2);
        }
        double f = 0.0;
#pragma unroll
        for (int d = 0; d < SD; ++d)
          if (d < nx) {
            double g = 0.0;
#pragma unroll
            for (int c = 0; c <= d; ++c) g = __builtin_fma(St[m][d * (d + 1) / 2 + c], dl[c], g);
            f = __builtin_fma(g, dl[d], f);
          }
        const double v = (jb + jj < r1) ? sf2 * gpk_exp_neg(-0.5 * d2) : 0.0;
        ks[m][jj] = v;
        kq[m][jj] = v * f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TRACE_OUTS; ++u) {
      const int t = tid + 256 * u;
      if (t < MP) {
        const int m = t / P, p = t - m * P;
        double sT = accT[u], sS = accS[u];
#pragma unroll 8
        for (int jj = 0; jj < HJ; ++jj) {
          sT = __builtin_fma(kq[m][jj], al[jj][p], sT);
          sS = __builtin_fma(ks[m][jj], al[jj][p], sS);
        }
        accT[u] = sT;
        accS[u] = sS;
      }
    }
  }
  double* slot = shares + ((long long)blockIdx.x * gridDim.y * MP + (long long)b * MP) * 2;
#pragma unroll
  for (int u = 0; u < TRACE_OUTS; ++u) {
    const int t = tid + 256 * u;
    if (t < MP) {
      slot[2 * t] = accT[u];
      slot[2 * t + 1] = accS[u];
    }
  }
}

// ---- H w of the mean's input Hessian (K11, gradient of a horizon cost): the first launch of a backward propagation stage ----------
// The product of small_hess_kernel's result (per unit of the RAW query) with one vector per (query, output), formed without the
// Hessian.  With delta_mj = (z_m - x_j) / ls as above, s_d = in_scale_d ls_d (this model's own length-scales) and wh = w / s:
//   (H_mp w)_e = y_std[p] / s_e (sum_j k*_mj alpha_jp delta_mje (delta_mj . wh) - wh_e sum_j k*_mj alpha_jp)
// - D + 1 sums per (query, output).  w is a row of G = Lam A Sg, the sensitivity of the cost to A_h (gpk_propagate.hip): every
// workgroup forms the rows it needs from the chain's device buffers (SmallHvp), query by query through LDS, so that no launch
// precedes this one.  The workgroups take small_hess_kernel's rows (hess_rows(Np), at most 64 workgroups per model) in its
// rounds of HJ rows, K* recomputed from the device query rows.  The outputs are cut into slices of hvp_slice(M, nx, P) over the
// third grid dimension, so that the slice's wh (M x slice x nx) stays within HVP_W doubles of LDS.  The workgroup writes
// its finished share y_std / s_e (sum_e - wh_e S) to its own slot, shares[(group * E + e) * D + d] with e = (model * M + m) * P + p
// and E = B M P.  No ticket and no last workgroup: the chain's adjoint launch adds the slots in workgroup order.  Rows past N
// enter as zeros, a workgroup past the last row writes zeros, every slot is written, and rows, rounds and the order of every
// sum depend on (Np, M, P, D, nx) alone.
constexpr int HVP_W = 4096;
constexpr int HVP_OUTS = 2;        // (query, output) pairs per thread: M * slice <= 512
__host__ __device__ inline int hvp_slice(int M, int nx, int P) {
  const int n = HVP_W / (M * nx);      // M nx <= 512: at least 8
  return n > P ? P : n;
}

__global__ __launch_bounds__(256) void small_hvp_kernel(SmallK k, SmallHvp c, long long N, long long Np, int D, int P,
                                                        const double* __restrict__ Xq, int M, double* shares) {
  __shared__ double q[SQ][SD + 1];
  __shared__ double xs[HJ][SD + 1];
  __shared__ double al[HJ][SP + 1];
  __shared__ double ks[SQ][HJ + 1];
  __shared__ double wh[HVP_W];
  __shared__ double lin_s[SD * SD];
  __shared__ double ls[SD], sl[SD];
  const int b = blockIdx.y, tid = threadIdx.x;
  const double* __restrict__ X = k.X[b];
  const double* __restrict__ alpha = k.alpha[b];
  const double sf2 = k.sf2[b];
  const int nx = c.nx;
  const int ps = hvp_slice(M, nx, P), p0 = blockIdx.z * ps, np = min(P, p0 + ps) - p0, MPs = M * np;
  const long long rows = hess_rows(Np);
  const long long r0 = (long long)blockIdx.x * rows, r1 = min(N, r0 + rows);
  if (tid < SD) {
    ls[tid] = k.ls[b][tid];
    sl[tid] = c.in_scale[tid] * k.ls[b][tid];
  }
  for (int e = tid; e < nx * D; e += 256) lin_s[e] = c.lin[e];
  __syncthreads();
  for (int e = tid; e < M * SD; e += 256) {
    const int m = e / SD, d = e % SD;
    q[m][d] = d < D ? Xq[m * D + d] / ls[d] : 0.0;
  }
  // wh of (query m, output p0 + pp): row coord_of[output] of Lam A Sg, divided by s.  One thread per entry (m, pp, j), all
  // queries at once (the operands come from L2 with many loads in flight, not query by query): first T = Lam[co, :] A into
  // the buffer, then T Sg over it.  Every sum runs over the coordinates in order.
  {
    const int W = MPs * nx, npn = np * nx;
    for (int e = tid; e < W; e += 256) {
      const int m = e / npn, rem = e - m * npn, pp = rem / nx, j = rem - pp * nx;
      const double* Lrow = c.Lam + ((long long)m * nx + c.coord_of[b * P + p0 + pp]) * nx;
      double t = 0.0;
      for (int i = 0; i < nx; ++i) {
        const int o = c.model_of[i];
        double a = (i == j ? 1.0 : 0.0) + lin_s[i * D + j];
        if (o >= 0) {
          const double g = c.sjac[(long long)(o * c.so + m * c.sm) * D + j];
          a += c.scaled ? g / c.in_scale[j] : g;
        }
        t = __builtin_fma(Lrow[i], a, t);
      }
      wh[(m * ps + pp) * nx + j] = t;
    }
    __syncthreads();
    double wr[HVP_W / 256];
#pragma unroll
    for (int u = 0; u < HVP_W / 256; ++u) {
      const int e = tid + 256 * u;
      wr[u] = 0.0;
      if (e < W) {
        const int m = e / npn, rem = e - m * npn, pp = rem / nx, j = rem - pp * nx;
        const double* T = wh + (m * ps + pp) * nx;
        const double* Sg = c.Sg + (long long)m * nx * nx + j;
        double w = 0.0;
        for (int i = 0; i < nx; ++i) w = __builtin_fma(T[i], Sg[i * nx], w);
        wr[u] = w / sl[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < HVP_W / 256; ++u) {
      const int e = tid + 256 * u;
      if (e < W) {
        const int m = e / npn, rem = e - m * npn, pp = rem / nx, j = rem - pp * nx;
        wh[(m * ps + pp) * nx + j] = wr[u];
      }
    }
  }
  __syncthreads();
  double acc[HVP_OUTS][SD + 1];
#pragma unroll
  for (int u = 0; u < HVP_OUTS; ++u)
#pragma unroll
    for (int d = 0; d <= SD; ++d) acc[u][d] = 0.0;
  for (long long jb = r0; jb < r1; jb += HJ) {
    __syncthreads();
    for (int e = tid; e < HJ * SD; e += 256) {
      const int jj = e / SD, d = e % SD;
      xs[jj][d] = (d < D && jb + jj < r1) ? X[(jb + jj) * D + d] / ls[d] : 0.0;
    }
    for (int e = tid; e < HJ * P; e += 256) {
      const int jj = e / P, p = e - jj * P;
      al[jj][p] = (jb + jj < r1) ? alpha[(jb + jj) * P + p] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TRACE_PAIRS; ++u) {
      const int e = tid + 256 * u, m = e / HJ, jj = e % HJ;
      if (m < M) {
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < SD; ++d) {
          const double dl = q[m][d] - xs[jj][d];
          d2 = __builtin_fma(dl, dl, d2);
        }
        ks[m][jj] = (jb + jj < r1) ? sf2 * gpk_exp_neg(-0.5 * d2) : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < HVP_OUTS; ++u) {
      const int t = tid + 256 * u;
      if (t < MPs) {
        const int m = t / np, pp = t - m * np;
        double qm[SD], wm[SD];      // (wm: zeros from nx on, so the product below takes no select)
#pragma unroll
        for (int d = 0; d < SD; ++d) {
          qm[d] = q[m][d];
          wm[d] = d < nx ? wh[(m * ps + pp) * nx + d] : 0.0;
        }
        for (int jj = 0; jj < HJ; ++jj) {
          const double cf = ks[m][jj] * al[jj][p0 + pp];
          double dl[SD], dot = 0.0;
#pragma unroll
          for (int d = 0; d < SD; ++d) {
            dl[d] = qm[d] - xs[jj][d];
            dot = __builtin_fma(dl[d], wm[d], dot);
          }
          const double cd = cf * dot;
#pragma unroll
          for (int d = 0; d < SD; ++d) acc[u][d] = __builtin_fma(cd, dl[d], acc[u][d]);
          acc[u][SD] += cf;
        }
      }
    }
  }
  const long long E = (long long)gridDim.y * M * P;
#pragma unroll
  for (int u = 0; u < HVP_OUTS; ++u) {
    const int t = tid + 256 * u;
    if (t < MPs) {
      const int m = t / np, pp = t - m * np, o = b * P + p0 + pp;
      const double* w = wh + (m * ps + pp) * nx;
      double* slot = shares + ((long long)blockIdx.x * E + ((long long)b * M + m) * P + p0 + pp) * D;
#pragma unroll
      for (int d = 0; d < SD; ++d)
        if (d < D) slot[d] = k.ystd[o] * (acc[u][d] - (d < nx ? w[d] : 0.0) * acc[u][SD]) / sl[d];
    }
  }
}

// NMB = 1: up to 16 queries, 2: up to 32.  8 waves: wave w takes the 64-wide k-chunks w, w + 8, ..., the loads of
// the next one in flight while the current one is multiplied.
constexpr int VW = 8;

template <int NMB>
struct VFrag { d2v a[8], b[NMB][8]; };

template <int NMB>
__device__ __forceinline__ void vload(VFrag<NMB>& f, const double* wp, const double* const (&kp)[NMB], long long kc) {
#pragma unroll
  for (int s = 0; s < 8; ++s) f.a[s] = *reinterpret_cast<const d2v*>(wp + kc + 8 * s);
#pragma unroll
  for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
    for (int s = 0; s < 8; ++s) f.b[mb][s] = *reinterpret_cast<const d2v*>(kp[mb] + kc + 8 * s);
}

template <int NMB>
__device__ __forceinline__ void vmul(const VFrag<NMB>& f, long long kc, int kq, long long row, d4 (&acc)[NMB]) {
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const long long k0 = kc + 8 * s + 2 * kq;
    const double ax = (k0 <= row) ? f.a[s].x : 0.0;            // strictly-upper entries never enter
    const double ay = (k0 + 1 <= row) ? f.a[s].y : 0.0;
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb) {
      acc[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, f.b[mb][s].x, acc[mb], 0, 0, 0);
      acc[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay, f.b[mb][s].y, acc[mb], 0, 0, 0);
    }
  }
}

// This workgroup's 16 rows of V = W K*^T (rows blockIdx.x * SR ..), one partial per wave: red[w][mb][row][query].  The
// barrier after the stores is the last thing it does.
template <int NMB>
__device__ __forceinline__ void small_v_rows(const double* __restrict__ W, long long ldw, long long Np, const double* Ks, int M,
                                             double (&red)[VW][NMB][16][17]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, kq = lane >> 4;
  const long long r0 = (long long)blockIdx.x * SR, row = r0 + i;
  const long long kend = min(Np, (r0 + SR + 63) / 64 * 64);   // the rows' diagonal, rounded up to the chunk
  const int nch = (int)(kend / 64);
  const double* wp = W + row * ldw + 2 * kq;
  const double* kp[NMB];
#pragma unroll
  for (int mb = 0; mb < NMB; ++mb) kp[mb] = Ks + (long long)min(16 * mb + i, M - 1) * Np + 2 * kq;  // columns >= M: unused
  d4 acc[NMB];
#pragma unroll
  for (int mb = 0; mb < NMB; ++mb) acc[mb] = d4{0.0, 0.0, 0.0, 0.0};
  // Chunk of 64 k: step s covers k = 8 s + 2 kq + {0, 1} for kq = 0..3 -- one 16-byte load per lane and
  // operand, 64 contiguous bytes per row and step; the two halves feed two MFMAs.
  VFrag<NMB> f0, f1;
  if (w < nch) vload<NMB>(f0, wp, kp, (long long)w * 64);
  for (int c = w; c < nch; c += 2 * VW) {
    const bool n1 = c + VW < nch, n2 = c + 2 * VW < nch;
    if (n1) vload<NMB>(f1, wp, kp, (long long)(c + VW) * 64);
    vmul<NMB>(f0, (long long)c * 64, kq, row, acc);
    if (n2) vload<NMB>(f0, wp, kp, (long long)(c + 2 * VW) * 64);
    if (n1) vmul<NMB>(f1, (long long)(c + VW) * 64, kq, row, acc);
  }
  // accumulator map: column = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][mb][kq + 4 * r][i] = acc[mb][r];
  __syncthreads();
}

// V[row r][query 16 mb + c] of this workgroup: the waves' partials, added in wave order
template <int NMB>
__device__ __forceinline__ double small_v_sum(const double (&red)[VW][NMB][16][17], int mb, int r, int c) {
  double v = 0.0;
#pragma unroll
  for (int u = 0; u < VW; ++u) v += red[u][mb][r][c];
  return v;
}

// GRAD (small_var_grad_kernel): the launch also stores its rows of V (Vs: per model Np x SQ, columns < 16 NMB written) for
// small_wtv_grad_kernel, and workgroup 1 adds the mean Jacobian's shares of the previous launch.  The body is shared;
// small_var_kernel keeps its signature and its launches.
// TWO (the sparse model): blockIdx.y is 2 * model + the inverse FACTOR (0: Wuu,
// 1: WSigma); one model with P outputs, or B models with one each.  Both factors of a model read its K* and its mean / Jacobian
// shares (model slot o); each has its own shares (and rows of V, slot 2 o + f); ONE ticket count per model runs over the
// workgroups of both, and the model's last one adds each factor's shares in the order above and writes
// var[m][p] = max((kss - t0) - (0 - t1), floor) y_std[p]^2.
// GRAD = 2 (small_var_jac_kernel, the propagation chain's stage): the Jacobian is finished as with GRAD = 1, V is not stored.
template <int NMB, int GRAD, bool TWO>
__device__ __forceinline__ void small_var_body(SmallK k, long long ldw, long long Np, const double* Ks,
                                                            int M, int P, double floor_, const double* pmean,
                                                            unsigned mean_shares, double* pvar, unsigned* counter,
                                                            double* mean_out, double* var_out, double* Vs,
                                                            const double* pjac, int D, double* dmean_out) {
  __shared__ double red[VW][NMB][16][17];
  __shared__ double sq[NMB][16][17];
  const int b = blockIdx.y;                    // the model, or 2 * model + factor
  const int o = TWO ? b >> 1 : b;              // the model slot of everything but W and the factor's own shares
  const bool lead = TWO ? (b & 1) == 0 : true; // the factor whose workgroups 0 and 1 finish the means and the Jacobian
  const double* __restrict__ W = (TWO && (b & 1)) ? k.W2[o] : k.W[o];
  const double kss = k.kss[o];
  Ks += (long long)o * SQ * Np;
  pmean += (long long)o * mean_shares * (SQ * SP);
  double* const pvar0 = pvar + (long long)(2 * o) * gridDim.x * SQ;     // (TWO) the shares of this model's factor 0, then 1
  pvar += (long long)b * gridDim.x * SQ;
  mean_out += (long long)o * M * P;
  var_out += (long long)o * M * (TWO ? P : 1);
  counter += o;
  if constexpr (GRAD == 1) Vs += (long long)b * Np * SQ;
  if constexpr (GRAD != 0) {
    pjac += (long long)o * mean_shares * (M * P * D);
    dmean_out += (long long)o * M * P * D;
  }
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * SR;
  small_v_rows<NMB>(W, ldw, Np, Ks, M, red);
  for (int e = tid; e < NMB * 256; e += 64 * VW) {
    const int mb = e >> 8, r = (e >> 4) & 15, c = e & 15;
    const double v = small_v_sum<NMB>(red, mb, r, c);
    sq[mb][r][c] = v * v;
    if constexpr (GRAD == 1) Vs[(r0 + r) * SQ + 16 * mb + c] = v;
  }
  __syncthreads();
  if (tid < NMB * 16) {
    const int mb = tid >> 4, c = tid & 15;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += sq[mb][r][c];
    pvar[(long long)blockIdx.x * SQ + tid] = s;
  }
  // The mean shares are complete since the previous launch: the workgroup with the shortest rows adds them up while
  // the others are still multiplying, off the critical path (scratch: the reduction buffer, free by now).
  static_assert(VW * 16 * 17 >= 4 * SQ * SP, "the reduction buffer doubles as the mean scratch");
  if (blockIdx.x == 0 && lead) finish_means(pmean, mean_shares, M, P, k.ymean + o * P, k.ystd + o * P, mean_out, tid, &red[0][0][0][0]);
  if constexpr (GRAD != 0) {
    if (blockIdx.x == 1 && lead) finish_jac(pjac, mean_shares, M, P, D, k.ystd + o * P, k.ls[o], dmean_out, tid, 64 * VW);
  }
  if (last_of(counter, (TWO ? 2u : 1u) * gridDim.x, tid)) {
    constexpr int NF = TWO ? 2 : 1;
    __shared__ double part[NF][2 * VW][SQ];
    const int m = tid & 31, pt = tid >> 5;
    if constexpr (!TWO) {
      part[0][pt][m] = (m < NMB * 16) ? sum_shares(pvar + m, pt, 2 * VW, gridDim.x, SQ) : 0.0;
    } else {
      double s0 = 0.0, s1 = 0.0;
      if (m < NMB * 16) sum_shares2(pvar0 + m, pvar0 + (long long)gridDim.x * SQ + m, pt, 2 * VW, gridDim.x, SQ, s0, s1);
      part[0][pt][m] = s0;
      part[1][pt][m] = s1;
    }
    __syncthreads();
    if constexpr (!TWO) {
      if (tid < M) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * VW; ++k) t += part[0][k][tid];
        var_out[tid] = fmax(kss - t, floor_);
      }
    } else {
      for (int e = tid; e < M * P; e += 64 * VW) {
        const int mq = e / P, p = e - mq * P;
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * VW; ++k) t0 += part[0][k][mq];
#pragma unroll
        for (int k = 0; k < 2 * VW; ++k) t1 += part[1][k][mq];
        const double ys = k.ystd[o * P + p];
        var_out[e] = fmax((kss - t0) - (0.0 - t1), floor_) * ys * ys;
      }
    }
  }
}

// TWO: the two-factor forms (the sparse model: blockIdx.y = 2 * model + inverse factor; var_out is M x P, already times y_std[p]^2)
template <int NMB, bool TWO>
__global__ __launch_bounds__(64 * VW) void small_var_kernel(SmallK k, long long ldw, long long Np, const double* Ks,
                                                            int M, int P, double floor_, const double* pmean,
                                                            unsigned mean_shares, double* pvar, unsigned* counter,
                                                            double* mean_out, double* var_out) {
  small_var_body<NMB, 0, TWO>(k, ldw, Np, Ks, M, P, floor_, pmean, mean_shares, pvar, counter, mean_out, var_out, nullptr, nullptr, 0,
                              nullptr);
}
template <int NMB, bool TWO>
__global__ __launch_bounds__(64 * VW) void small_var_grad_kernel(SmallK k, long long ldw, long long Np, const double* Ks,
                                                                 int M, int P, double floor_, const double* pmean,
                                                                 unsigned mean_shares, double* pvar, unsigned* counter,
                                                                 double* mean_out, double* var_out, double* Vs,
                                                                 const double* pjac, int D, double* dmean_out) {
  small_var_body<NMB, 1, TWO>(k, ldw, Np, Ks, M, P, floor_, pmean, mean_shares, pvar, counter, mean_out, var_out, Vs, pjac, D,
                              dmean_out);
}

// mean + Jacobian + variance without the variance gradient (GPK_SMALL_JACVAR): small_var_grad_kernel without its store of V
template <int NMB>
__global__ __launch_bounds__(64 * VW) void small_var_jac_kernel(SmallK k, long long ldw, long long Np, const double* Ks, int M, int P,
                                                                double floor_, const double* pmean, unsigned mean_shares,
                                                                double* pvar, unsigned* counter, double* mean_out, double* var_out,
                                                                const double* pjac, int D, double* dmean_out) {
  small_var_body<NMB, 2, false>(k, ldw, Np, Ks, M, P, floor_, pmean, mean_shares, pvar, counter, mean_out, var_out, nullptr, pjac, D,
                                dmean_out);
}
// ... its two-factor form (the sparse model's stage): small_var_grad_kernel<NMB, true> without its store of V - blockIdx.y = 2 *
// model + inverse factor, one ticket count per model, var_out M x P (B x M for a batch) already times y_std^2
template <int NMB>
__global__ __launch_bounds__(64 * VW) void small_var_jac2_kernel(SmallK k, long long ldw, long long Np, const double* Ks, int M, int P,
                                                                 double floor_, const double* pmean, unsigned mean_shares,
                                                                 double* pvar, unsigned* counter, double* mean_out, double* var_out,
                                                                 const double* pjac, int D, double* dmean_out) {
  small_var_body<NMB, 2, true>(k, ldw, Np, Ks, M, P, floor_, pmean, mean_shares, pvar, counter, mean_out, var_out, nullptr, pjac, D,
                               dmean_out);
}

constexpr int CG = 16;                   // workgroups per first-level group of the covariance reduction
constexpr int CE = SQ * (SQ + 1) / 2;    // packed lower-triangle entries of a 32 x 32 share

// entry t of the packed lower triangle -> (i, j), i >= j
__device__ __forceinline__ void tri_index(int t, int& i, int& j) {
  i = (int)((__builtin_sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  while (i * (i + 1) / 2 > t) --i;
  j = t - i * (i + 1) / 2;
}

// Posterior covariance of M <= 32 queries (model y = blockIdx.y): the rows of V as in small_var_kernel, then the workgroup's
// share of V^T V.  Per model: COV_COUNTERS ticket counters ([0] the top level, [1 + g] group g; all left at zero), pcov
// (gridDim.x x CE), gcov (groups x CE), cov_out (M x M).  A model's sums are grouped by Np and M alone: its block has the
// bits of that model served on its own.
constexpr int COV_GROUPS = (int)(GPK_SMALL_MAX_NP / SR / CG);
constexpr int COV_COUNTERS = 1 + COV_GROUPS;
constexpr int COV2_COUNTERS = 1 + 2 * COV_GROUPS;
// TWO (the sparse model): blockIdx.y is 2 * model + inverse factor.  Both factors of a model read its K* and
// mean shares; each has its own shares, group sums and group counters; per model COV2_COUNTERS counters ([0] the top level,
// [1 + f * COV_GROUPS + g] group g of factor f): the top level is ONE count over the groups of both factors, and the model's
// last group writes (k(a, b) - s0) + s1, mirrored.  Two ticket levels, each with its own last_of: a group's last workgroup reads its group's
// shares behind the group's ticket, the last group reads all group sums - of both factors - behind the top ticket.
template <int NMB, bool TWO>
__device__ __forceinline__ void small_cov_body(SmallK k, long long ldw, long long Np, const double* Ks, int M,
                                               int D, int P, const double* Xq,
                                               const double* pmean, unsigned mean_shares, double* pcov,
                                               double* gcov, unsigned* counters, double* mean_out,
                                               double* cov_out) {
  __shared__ double red[VW][NMB][16][17];
  __shared__ double vt[NMB * 16][17];          // this workgroup's rows of V, transposed: [query][row]
  __shared__ double qs[SQ][SD + 1];
  const int f = blockIdx.y;                    // the model, or 2 * model + factor
  const int y = TWO ? f >> 1 : f;              // the model slot of everything but W and the factor's own shares
  const int fac = TWO ? f & 1 : 0;
  const unsigned ng = (gridDim.x + CG - 1) / CG;
  const double* __restrict__ W = fac ? k.W2[y] : k.W[y];
  const double sf2 = k.sf2[y], noise = k.noise[y];
  Ks += (long long)y * SQ * Np;
  pmean += (long long)y * mean_shares * (SQ * SP);
  double* const gcov0 = gcov + (long long)(2 * y) * ng * CE;      // (TWO) the group sums of this model's factor 0, then 1
  pcov += (long long)f * gridDim.x * CE;
  gcov += (long long)f * ng * CE;
  unsigned* const top = counters + y * (TWO ? COV2_COUNTERS : COV_COUNTERS);
  counters = top + fac * COV_GROUPS;
  mean_out += (long long)y * M * P;
  cov_out += (long long)y * M * M;
  const int tid = threadIdx.x;
  small_v_rows<NMB>(W, ldw, Np, Ks, M, red);
  for (int e = tid; e < NMB * 256; e += 64 * VW) {
    const int mb = e >> 8, r = (e >> 4) & 15, c = e & 15;
    const double v = small_v_sum<NMB>(red, mb, r, c);
    vt[16 * mb + c][r] = (16 * mb + c < M) ? v : 0.0;     // (columns >= M repeat query M - 1: dropped)
  }
  __syncthreads();
  // the share: lower triangle of V_r^T V_r over this workgroup's 16 rows, packed
  constexpr int NE = NMB * 16 * (NMB * 16 + 1) / 2;
  for (int t = tid; t < NE; t += 64 * VW) {
    int a, b;
    tri_index(t, a, b);
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) s = __builtin_fma(vt[a][r], vt[b][r], s);
    pcov[(long long)blockIdx.x * CE + t] = s;
  }
  // the mean shares are complete since the previous launch (as in small_var_kernel; scratch: the reduction buffer)
  static_assert(VW * 16 * 17 >= 4 * SQ * SP, "the reduction buffer doubles as the mean scratch");
  if (blockIdx.x == 0 && fac == 0) finish_means(pmean, mean_shares, M, P, k.ymean + y * P, k.ystd + y * P, mean_out, tid, &red[0][0][0][0]);
  const unsigned g = blockIdx.x / CG, g0 = g * CG, g1 = min(g0 + CG, gridDim.x);
  if (!last_of(counters + 1 + g, g1 - g0, tid)) return;
  for (int t = tid; t < NE; t += 64 * VW) gcov[(long long)g * CE + t] = sum_shares(pcov + t, g0, 1, g1, CE);
  if (!last_of(top, (TWO ? 2u : 1u) * ng, tid)) return;
  for (int e = tid; e < M * D; e += 64 * VW) qs[e / D][e % D] = Xq[e] / k.ls[y][e % D];
  __syncthreads();
  for (int t = tid; t < NE; t += 64 * VW) {
    int a, b;
    tri_index(t, a, b);
    if (a >= M) continue;
    double s, s2 = 0.0;
    if constexpr (TWO) sum_shares2(gcov0 + t, gcov0 + (long long)ng * CE + t, 0, 1, ng, CE, s, s2);
    else s = sum_shares(gcov + t, 0, 1, ng, CE);
    double kv;
    if (a == b) {
      kv = sf2 + noise;
    } else {
      double d2 = 0.0;
#pragma unroll
      for (int d = 0; d < SD; ++d)
        if (d < D) {
          const double df = qs[a][d] - qs[b][d];
          d2 = __builtin_fma(df, df, d2);
        }
      kv = sf2 * gpk_exp_neg(-0.5 * d2);
    }
    double v = kv - s;
    if constexpr (TWO) v += s2;
    cov_out[(long long)a * M + b] = v;
    cov_out[(long long)b * M + a] = v;
  }
}

template <int NMB, bool TWO>
__global__ __launch_bounds__(64 * VW) void small_cov_kernel(SmallK k, long long ldw, long long Np, const double* Ks, int M,
                                                            int D, int P, const double* Xq,
                                                            const double* pmean, unsigned mean_shares, double* pcov,
                                                            double* gcov, unsigned* counters, double* mean_out,
                                                            double* cov_out) {
  small_cov_body<NMB, TWO>(k, ldw, Np, Ks, M, D, P, Xq, pmean, mean_shares, pcov, gcov, counters, mean_out, cov_out);
}

// Variance gradient of M <= 32 queries (model = blockIdx.z), after small_cross_mean_kernel (K*: Ks, query-major) and
// small_var_grad_kernel (V: Vs, Np x SQ): 16 columns of W per workgroup.  C[j][m] = sum_{r >= j} W[r][j] V[r][m] on the
// vector ALU (thread = column jl, query half mh, row group rg of 16; the row groups are added in a fixed order through LDS),
// then the workgroup's share of sum_j k*_mj C_jm (x_jd - q_md) / ls_d (pdv: gridDim.x x M * D); the last workgroup adds the
// shares in order and writes dvar[m][d] = -2 / ls_d * sum.  pdv: gridDim.x * gridDim.y shares per model; counter: one per model.
constexpr unsigned WTV_MAX_ROW_CHUNKS = 4;
constexpr int GW = 16, GRG = 16, GT = GW * 2 * GRG;      // 512 threads: column jl, query half mh, row group rg
// TWO (the sparse model): blockIdx.z is 2 * model + inverse factor: the model's K*, inputs and
// queries, the factor's own V and shares; per model ONE ticket count over the workgroups of both factors, and the model's last
// one adds each factor's shares as above and writes dvar[m][d] = -2 / ls_d * (s0 - s1).
template <bool TWO>
__device__ __forceinline__ void small_wtv_grad_body(SmallK k, long long ldw, long long N, long long Np, int D,
                                                    const double* __restrict__ Ks_all, const double* __restrict__ Vs_all,
                                                    const double* __restrict__ Xq, int M, double* pdv,
                                                    unsigned* counter, double* dvar_out) {
  __shared__ double red[GRG][GW][17];
  __shared__ double cm[GW][SQ + 1];
  __shared__ double xs[GW][SD + 1];
  __shared__ double qs[SQ][SD + 1];
  __shared__ double half[2][SQ * SD];
  const int b = blockIdx.z;                    // the model, or 2 * model + factor
  const int o = TWO ? b >> 1 : b;              // the model slot of everything but W, V and the factor's own shares
  const double* __restrict__ W = (TWO && (b & 1)) ? k.W2[o] : k.W[o];
  const double* __restrict__ X = k.X[o];
  const double* ls = k.ls[o];
  const double* __restrict__ Ks = Ks_all + (long long)o * SQ * Np;
  const double* __restrict__ Vs = Vs_all + (long long)b * Np * SQ;
  double* const pdv0 = pdv + (long long)(2 * o) * gridDim.x * gridDim.y * (M * D);     // (TWO) this model's factor 0, then 1
  pdv += (long long)b * gridDim.x * gridDim.y * (M * D);
  dvar_out += (long long)o * M * D;
  counter += o;
  const int tid = threadIdx.x, jl = tid & 15, mh = (tid >> 4) & 1, rg = tid >> 5;
  const long long j0 = (long long)blockIdx.x * GW, j = j0 + jl;
  // queries and this workgroup's training rows, divided by the length-scales
  for (int e = tid; e < M * D; e += GT) qs[e / D][e % D] = Xq[e] / ls[e % D];
  for (int e = tid; e < GW * D; e += GT) {
    const int jj = e / D, d = e - jj * D;
    xs[jj][d] = (j0 + jj < N) ? X[(j0 + jj) * D + d] / ls[d] : 0.0;
  }
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0;
  const bool active = 16 * mh < M;                    // (M <= 16: the second query half holds nothing)
  if (active) {
    // rows r = j0 + rg + GRG * it, four at a time: their loads go out together (the loop is a chain of L2 latencies);
    // rows beyond the end are clamped to the last one and enter with weight zero
    // (blockIdx.y: the rows below the diagonal cut into gridDim.y equal chunks - C is linear in them, so every chunk simply
    // contributes its own share; small models have too few column blocks to fill the device otherwise)
    const long long span = ((Np - j0 + gridDim.y - 1) / gridDim.y + GRG - 1) / GRG * GRG;
    const long long rb = j0 + blockIdx.y * span, re = min(Np, rb + span);
    for (long long r0 = rb + rg; r0 < re; r0 += 4 * GRG) {
      double w[4];
      d2v v[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long r = r0 + u * GRG, rc = min(r, Np - 1);
        w[u] = W[rc * ldw + j];
        if (r >= re || r < j) w[u] = 0.0;             // strictly-upper entries never enter
        const d2v* vp = reinterpret_cast<const d2v*>(Vs + rc * SQ + 16 * mh);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[u][i] = vp[i];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          acc[2 * i] = __builtin_fma(w[u], v[u][i].x, acc[2 * i]);
          acc[2 * i + 1] = __builtin_fma(w[u], v[u][i].y, acc[2 * i + 1]);
        }
    }
  }
  // the row groups are added in order, one query half at a time (the buffer holds 16 queries)
  for (int hq = 0; hq < 2; ++hq) {
    __syncthreads();
    if (mh == hq) {
#pragma unroll
      for (int i = 0; i < 16; ++i) red[rg][jl][i] = acc[i];
    }
    __syncthreads();
    if (tid < GW * 16) {
      const int jj = tid >> 4, i = tid & 15, m = 16 * hq + i;
      double v = 0.0;
#pragma unroll
      for (int u = 0; u < GRG; ++u) v += red[u][jj][i];
      cm[jj][m] = (m < M) ? v : 0.0;                  // (columns >= M of V: duplicates of query M - 1 or unwritten)
    }
  }
  __syncthreads();
  const int MD = M * D;
  for (int t = tid; t < MD; t += GT) {
    const int m = t / D, d = t - m * D;
    const double qd = qs[m][d];
    double s = 0.0;
#pragma unroll
    for (int jj = 0; jj < GW; ++jj) s = __builtin_fma(Ks[(long long)m * Np + j0 + jj] * cm[jj][m], xs[jj][d] - qd, s);
    pdv[((long long)blockIdx.y * gridDim.x + blockIdx.x) * MD + t] = s;
  }
  if (last_of(counter, (TWO ? 2u : 1u) * gridDim.x * gridDim.y, tid)) {
    // each entry's shares in two halves (thread halves), each half in share order with sixteen loads in flight - the chain
    // of misses is the cost - then half 0 + half 1
    constexpr int NF = TWO ? 2 : 1;
    static_assert(GRG * GW * 17 >= 2 * SQ * SD, "the row groups' buffer doubles as the second factor's halves");
    double (*half1)[SQ * SD] = reinterpret_cast<double (*)[SQ * SD]>(&red[0][0][0]);     // (free since the barriers above)
    const unsigned ns = gridDim.x * gridDim.y, h0 = (ns + 1) / 2;
    for (int base = 0; base < MD; base += GT / 2) {
      const int part = tid / (GT / 2), t = base + tid - part * (GT / 2);
      const unsigned g0 = part ? h0 : 0, g1 = part ? ns : h0;
      if (t < MD) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const double* pf = TWO ? pdv0 + (long long)f * ns * MD : pdv;
          double sum = 0.0;
          for (unsigned g = g0; g < g1; g += 16) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
              v[u] = pf[(long long)min(g + u, g1 - 1) * MD + t];
              if (g + u >= g1) v[u] = 0.0;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) sum += v[u];
          }
          (f ? half1 : half)[part][t] = sum;
        }
      }
      __syncthreads();
      if (part == 0 && t < MD) {
        if constexpr (TWO)
          dvar_out[t] = -2.0 / ls[t % D] * ((half[0][t] + half[1][t]) - (half1[0][t] + half1[1][t]));
        else
          dvar_out[t] = -2.0 / ls[t % D] * (half[0][t] + half[1][t]);
      }
    }
  }
}

template <bool TWO>
__global__ __launch_bounds__(GT) void small_wtv_grad_kernel(SmallK k, long long ldw, long long N, long long Np, int D,
                                                            const double* __restrict__ Ks_all, const double* __restrict__ Vs_all,
                                                            const double* __restrict__ Xq, int M, double* pdv,
                                                            unsigned* counter, double* dvar_out) {
  small_wtv_grad_body<TWO>(k, ldw, N, Np, D, Ks_all, Vs_all, Xq, M, pdv, counter, dvar_out);
}

// The device work area of one call: offsets (in doubles) of the sub-buffers the launches below hand to the kernels, and
// their total - the one place that lays it out.  Every call has K* and the mean shares; the rest follows what it computes.
// B models with F inverse factors each (F = 2: the two-factor kernels, slot 2 * model + factor): BF = B * F.
struct SmallWork {
  size_t Ks;             // B x SQ x Np
  size_t pmean;          // B x ga x (SQ * SP)
  size_t pvar;           // BF x gb x SQ                            (predict, grad)
  size_t pjac;           // B x ga x (M * P * D)                    (grad, jacvar)
  size_t Vs;             // BF x Np x SQ                            (grad)
  size_t pdv;            // BF x (gb x row chunks) x (M * D)        (grad)
  size_t pcov, gcov;     // BF x gb x CE, BF x (gb / CG rounded up) x CE   (cov)
  size_t phess;          // B x hess_groups(Np) x (M * P * (D (D + 1) / 2 + 1))   (hess)
  size_t total;
};
// workgroups per model of small_hess_kernel: at most 64, a function of Np alone
unsigned hess_groups(int64_t Np) { return (unsigned)((Np + hess_rows(Np) - 1) / hess_rows(Np)); }
SmallWork small_work(int call, int64_t Np, int B, int64_t M, int D, int P, int F = 1) {
  const size_t ga = (size_t)(Np / SJ), gb = (size_t)(Np / SR), BF = (size_t)B * F;
  SmallWork w{};
  size_t at = 0;
  auto take = [&at](size_t doubles) { const size_t off = at; at += doubles; return off; };
  w.Ks = take((size_t)B * SQ * Np);
  w.pmean = take((size_t)B * ga * (SQ * SP));
  if (call == GPK_SMALL_COV) {
    w.pcov = take(BF * gb * CE);
    w.gcov = take(BF * ((gb + CG - 1) / CG) * CE);
  } else {
    w.pvar = take(BF * gb * SQ);
  }
  if (call == GPK_SMALL_GRAD) {
    w.pjac = take((size_t)B * ga * (size_t)(M * P * D));
    w.Vs = take(BF * Np * SQ);
    w.pdv = take(BF * gb * WTV_MAX_ROW_CHUNKS * (size_t)(M * D));
  } else if (call == GPK_SMALL_JACVAR) {
    w.pjac = take((size_t)B * ga * (size_t)(M * P * D));
  } else if (call == GPK_SMALL_HESS) {
    w.pjac = take((size_t)B * ga * (size_t)(M * P * D));
    w.phess = take((size_t)B * hess_groups(Np) * (size_t)(M * P * (D * (D + 1) / 2 + 1)));
  }
  w.total = at;
  return w;
}

// Checks the models' pointers and length-scales and fills the kernels' parameter block.  factors: the call forms V = W K*^T
// (otherwise the block's W stay null); kss goes in with a variance, noise with the covariance.  `name` prefixes the messages.
int small_params(gpk_handle h, const std::string& name, const ServeModels& m, bool factors, bool cov, SmallK& k) {
  for (int b = 0; b < m.B; ++b) {
    GPK_REQUIRE(h, m.X[b] && m.alpha[b], name + ": null model pointer");
    k.X[b] = m.X[b]; k.alpha[b] = m.alpha[b];
    for (int f = 0; factors && f < m.F; ++f) {
      const double* W = m.W[f][b];
      GPK_REQUIRE(h, W, name + ": null model pointer");
      GPK_REQUIRE(h, ((uintptr_t)W % 16) == 0, name + ": the inverse factor must be 16-byte aligned");
      (f ? k.W2 : k.W)[b] = W;
    }
    for (int d = 0; d < 16; ++d) k.ls[b][d] = 1.0;
    for (int d = 0; d < m.D; ++d) {
      GPK_REQUIRE(h, m.ls[b * m.D + d] > 0.0, "length-scales must be positive");
      k.ls[b][d] = m.ls[b * m.D + d];
    }
    k.sf2[b] = m.sf2[b];
    k.kss[b] = (factors && !cov) ? m.kss[b] : 0.0;
    k.noise[b] = cov ? m.noise[b] : 0.0;
  }
  for (int o = 0; o < m.B * m.P; ++o) { k.ymean[o] = m.y_mean[o]; k.ystd[o] = m.y_std[o]; }
  return GPK_OK;
}

// the zero-initialised ticket counters of the covariance reduction and of small_wtv_grad_kernel, allocated on first use
int ensure_cov_counters(gpk_handle h) {
  if (h->d_cov_count) return GPK_OK;
  GPK_CHECK_HIP(h, hipMalloc((void**)&h->d_cov_count, GPK_SMALL_COV_COUNTERS * sizeof(unsigned)));
  GPK_CHECK_HIP(h, hipMemsetAsync(h->d_cov_count, 0, GPK_SMALL_COV_COUNTERS * sizeof(unsigned), h->stream));
  return GPK_OK;
}
static_assert(COV_COUNTERS == 65, "one top-level counter and one per group of CG workgroups at GPK_SMALL_MAX_NP");
static_assert(COV2_COUNTERS == 129, "two-factor form: one top-level counter per model and one per group of either factor");
static_assert(GPK_SMALL_COV_COUNTERS >= GPK_SMALL_MAX_MODELS * COV_COUNTERS, "counters of the covariance reduction, per model");
// the ticket counters of small_wtv_grad_kernel (one per model): the last GPK_SMALL_MAX_MODELS of h->d_cov_count
constexpr int WTV_COUNTER0 = GPK_SMALL_COV_COUNTERS - GPK_SMALL_MAX_MODELS;
static_assert(WTV_COUNTER0 >= GPK_SMALL_MAX_MODELS * COV_COUNTERS, "the covariance reduction's counters come first");
// the two-factor forms (F = 2): model b takes slot b of the parameter block (its second factor: W2[b]), of the
// single ticket counts and of the work area's per-model shares; (model b, factor f) takes slot 2 b + f of the per-factor shares
// and the group counters [b * COV2_COUNTERS + 1 + f * COV_GROUPS + g] of the covariance
static_assert(WTV_COUNTER0 >= GPK_SMALL_MAX_MODELS * COV2_COUNTERS,
              "per model the top counter and the group counters of both factors, then small_wtv_grad_kernel's");
static_assert(SR == GW, "small_wtv_grad_kernel takes as many columns of W per workgroup as small_var_kernel takes rows");

// The instantiation a launch takes: one or two 16-query column blocks (M <= 16 or not), one or two inverse factors.
auto var_kernel(int64_t M, int F) {
  return M <= 16 ? (F == 2 ? small_var_kernel<1, true> : small_var_kernel<1, false>)
                 : (F == 2 ? small_var_kernel<2, true> : small_var_kernel<2, false>);
}
auto var_grad_kernel(int64_t M, int F) {
  return M <= 16 ? (F == 2 ? small_var_grad_kernel<1, true> : small_var_grad_kernel<1, false>)
                 : (F == 2 ? small_var_grad_kernel<2, true> : small_var_grad_kernel<2, false>);
}
auto cov_kernel(int64_t M, int F) {
  return M <= 16 ? (F == 2 ? small_cov_kernel<1, true> : small_cov_kernel<1, false>)
                 : (F == 2 ? small_cov_kernel<2, true> : small_cov_kernel<2, false>);
}
auto var_jac_kernel(int64_t M, int F) {
  return M <= 16 ? (F == 2 ? small_var_jac2_kernel<1> : small_var_jac_kernel<1>)
                 : (F == 2 ? small_var_jac2_kernel<2> : small_var_jac_kernel<2>);
}
auto wtv_grad_kernel(int F) { return F == 2 ? small_wtv_grad_kernel<true> : small_wtv_grad_kernel<false>; }

}  // namespace

size_t gpk_small_work_doubles(int call, int64_t Np, int B, int64_t M, int D, int P, int F) {
  return small_work(call, Np, B, M, D, P, F).total;
}

bool gpk_small_ok(int64_t Np, int D, int P, int64_t M) {
  return M >= 1 && M <= SQ && D >= 1 && D <= SD && P >= 1 && P <= SP && Np <= GPK_SMALL_MAX_NP;
}

int gpk_small_launch(gpk_handle h, int call, const ServeModels& m, const double* Xq, int64_t M, double* work, const ServeOut& out) {
  // jv: the first launch of a gradient call, then the variance launch that also finishes the Jacobian - no W^T V launch
  // hs: the gradient call's one launch for mean + Jacobian (no variance), then the Hessian launch
  const bool jv = call == GPK_SMALL_JACVAR, hs = call == GPK_SMALL_HESS, grad = call == GPK_SMALL_GRAD || jv || hs,
             cov = call == GPK_SMALL_COV;
  GPK_REQUIRE(h, call == GPK_SMALL_PREDICT || grad || cov, "small-batch launch: unknown call");
  const std::string name(cov ? "small cov" : jv ? "small jacvar" : hs ? "small hess" : grad ? "small grad" : "small predict");
  GPK_REQUIRE(h, !hs || (out.hess && out.dmean && !out.var && !out.dvar), name + ": mean, Jacobian and Hessian, no variance");
  const int B = m.B, D = m.D, P = m.P, F = m.F;
  const long long N = m.N, Np = gpk_padded(m.N), ldw = m.ldw;
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS && (B == 1 || P == 1) && (F == 1 || F == 2),
              name + ": 1 model, or up to 8 single-output models, of one or two inverse factors");
  GPK_REQUIRE(h, gpk_small_ok(Np, D, P, M), name + ": shape outside the small-batch path");
  GPK_REQUIRE(h, m.X && m.alpha && m.ls && m.sf2 && m.y_mean && m.y_std && Xq && work && out.mean, name + ": null pointer");
  GPK_REQUIRE(h, !grad || jv || (out.dmean && (out.var == nullptr) == (out.dvar == nullptr)), name + ": null pointer");
  GPK_REQUIRE(h, !jv || (out.dmean && out.var && !out.dvar), name + ": mean, variance and Jacobian, no variance gradient");
  GPK_REQUIRE(h, !cov || (out.cov && m.noise), name + ": null pointer");
  // the inverse factors enter with the variance (and its gradient) and with the covariance: the second and third launches
  const bool factors = cov || out.var;
  GPK_REQUIRE(h, !factors || (m.W[0] && (F == 1 || m.W[1]) && m.Np == Np && ldw >= Np && ldw % 2 == 0),
              name + ": needs the inverse factor of every model (both of the two-factor form), padded, with an even ldw >= Np");
  GPK_REQUIRE(h, cov || !factors || m.kss, name + ": null pointer");
  if (cov || hs || (grad && !jv && factors)) GPK_TRY(ensure_cov_counters(h));
  SmallK k{};
  GPK_TRY(small_params(h, name, m, factors, cov, k));
  const unsigned ga = (unsigned)(Np / SJ), gb = (unsigned)(Np / SR);
  // K*, the mean and the Jacobian shares once per model, every other share per (model, factor)
  const SmallWork wk = small_work(call, Np, B, M, D, P, F);
  double *Ks = work + wk.Ks, *pmean = work + wk.pmean, *pjac = work + wk.pjac;
  const dim3 g1(ga, B), g2(gb, B * F), b1(256), b2(64 * VW);
  if (h->gram_log) {   // option gram_log = 1: the form this call's launches take (the tests assert it per case); 0: not launched
    const unsigned wtv = 256 / (gb * (F == 2 ? 2u : (unsigned)B));
    fprintf(stderr, "GPKSMALL %s %d %d %lld %lld %d %d ga%u gb%u nmb%d rc%u hg%u sl%u\n", name.c_str() + 6, B, F, Np, (long long)M, D, P, ga,
            gb, factors ? (M <= 16 ? 1 : 2) : 0,
            (call == GPK_SMALL_GRAD && factors) ? (wtv < 1 ? 1u : wtv > WTV_MAX_ROW_CHUNKS ? WTV_MAX_ROW_CHUNKS : wtv) : 0u,
            hs ? hess_groups(Np) : 0u, hs ? (unsigned)((M * P + hess_slice(D) - 1) / hess_slice(D)) : 0u);
  }
  // The first launch.  Nothing follows (the mean, or the mean and its Jacobian): FINISH, and K* is not stored.
  if (grad)
    hipLaunchKernelGGL(factors ? small_cross_mean_jac_kernel<false> : small_cross_mean_jac_kernel<true>, g1, b1, 0, h->stream, k, N, Np,
                       D, P, Xq, (int)M, factors ? Ks : nullptr, pmean, h->d_count, out.mean, pjac, out.dmean);
  else
    hipLaunchKernelGGL(factors ? small_cross_mean_kernel<false> : small_cross_mean_kernel<true>, g1, b1, 0, h->stream, k, N, Np, D, P,
                       Xq, (int)M, factors ? Ks : nullptr, pmean, h->d_count, out.mean);
  GPK_LAUNCH_CHECK(h);
  unsigned* vcount = h->d_count + GPK_SMALL_MAX_MODELS;
  if (hs) {      // (the covariance reduction's ticket counters, all at zero between launches: no covariance launch runs in this call)
    const unsigned slices = (unsigned)((M * P + hess_slice(D) - 1) / hess_slice(D));
    static_assert(GPK_SMALL_COV_COUNTERS >= SQ * SP / (HESS_SLICE_ENTRIES / (HT_MAX + 1)) + GPK_SMALL_MAX_MODELS * SQ,
                  "one counter per (model, slice): at most 171 slices of one model, 11 of each of eight single-output models");
    hipLaunchKernelGGL(small_hess_kernel, dim3(hess_groups(Np), B, slices), b1, 0, h->stream, k, N, Np, D, P, Xq, (int)M,
                       work + wk.phess, h->d_cov_count, out.hess);
    GPK_LAUNCH_CHECK(h);
    return GPK_OK;
  }
  if (!factors) return GPK_OK;
  if (cov) {
    hipLaunchKernelGGL(cov_kernel(M, F), g2, b2, 0, h->stream, k, ldw, Np, Ks, (int)M, D, P, Xq, pmean, ga, work + wk.pcov,
                       work + wk.gcov, h->d_cov_count, out.mean, out.cov);
  } else if (jv) {
    hipLaunchKernelGGL(var_jac_kernel(M, F), g2, b2, 0, h->stream, k, ldw, Np, Ks, (int)M, P, m.floor_, pmean, ga, work + wk.pvar,
                       vcount, out.mean, out.var, pjac, D, out.dmean);
  } else if (!grad) {
    hipLaunchKernelGGL(var_kernel(M, F), g2, b2, 0, h->stream, k, ldw, Np, Ks, (int)M, P, m.floor_, pmean, ga, work + wk.pvar, vcount,
                       out.mean, out.var);
  } else {
    hipLaunchKernelGGL(var_grad_kernel(M, F), g2, b2, 0, h->stream, k, ldw, Np, Ks, (int)M, P, m.floor_, pmean, ga, work + wk.pvar,
                       vcount, out.mean, out.var, work + wk.Vs, pjac, D, out.dmean);
    GPK_LAUNCH_CHECK(h);
    // Row chunks of the W^T V launch: up to 4 per column block while that keeps the launch within one workgroup per CU (Np =
    // 1024: 64 x 4 for one model, 64 x 1 x 6 for six).  F = 1 counts the B models.  F = 2 counts the two factors of ONE model as
    // two models, whatever B is: a share is not linear in its chunk's bits (C enters an fma chain), so a count that fell with B
    // would give a model other bits inside a batch than alone; a function of Np alone keeps every sum's order fixed by (Np, M).
    unsigned rc = 256 / (gb * (F == 2 ? 2u : (unsigned)B));
    rc = rc < 1 ? 1 : (rc > WTV_MAX_ROW_CHUNKS ? WTV_MAX_ROW_CHUNKS : rc);
    hipLaunchKernelGGL(wtv_grad_kernel(F), dim3(gb, rc, B * F), dim3(GT), 0, h->stream, k, ldw, N, Np, D, Ks, work + wk.Vs, Xq, (int)M,
                       work + wk.pdv, h->d_cov_count + WTV_COUNTER0, out.dvar);
  }
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

unsigned gpk_small_trace_groups(int64_t Np) { return hess_groups(Np); }

int gpk_small_trace_launch(gpk_handle h, const ServeModels& m, const double* Xq, int64_t M, const double* Sg, int nx,
                           const double* in_scale, double* shares, double* trs) {
  const std::string name("small hess trace");
  const long long Np = gpk_padded(m.N);
  GPK_REQUIRE(h, m.B >= 1 && m.B <= GPK_SMALL_MAX_MODELS && (m.B == 1 || m.P == 1),
              name + ": 1 model, or up to 8 single-output models");
  GPK_REQUIRE(h, gpk_small_ok(Np, m.D, m.P, M) && nx >= 1 && nx <= m.D, name + ": shape outside the small-batch path");
  GPK_REQUIRE(h, m.X && m.alpha && m.ls && m.sf2 && m.y_mean && m.y_std && Xq && Sg && in_scale && shares && trs, name + ": null pointer");
  SmallK k{};
  GPK_TRY(small_params(h, name, m, false, false, k));
  Arr16 sc;
  for (int d = 0; d < 16; ++d) sc.v[d] = d < m.D ? in_scale[d] : 1.0;
  hipLaunchKernelGGL(small_hess_trace_kernel, dim3(hess_groups(Np), m.B), dim3(256), 0, h->stream, k, sc, (long long)m.N, Np, m.D, m.P, nx,
                     Xq, Sg, (int)M, shares, trs);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

int gpk_small_hvp_launch(gpk_handle h, const ServeModels& m, const double* Xq, int64_t M, const SmallHvp& c, double* shares) {
  const std::string name("small hvp");
  const long long Np = gpk_padded(m.N);
  GPK_REQUIRE(h, m.B >= 1 && m.B <= GPK_SMALL_MAX_MODELS && (m.B == 1 || m.P == 1),
              name + ": 1 model, or up to 8 single-output models");
  GPK_REQUIRE(h, gpk_small_ok(Np, m.D, m.P, M) && c.nx >= 1 && c.nx <= m.D, name + ": shape outside the small-batch path");
  GPK_REQUIRE(h, m.X && m.alpha && m.ls && m.sf2 && m.y_mean && m.y_std && Xq && c.Lam && c.Sg && c.sjac && c.lin && shares,
              name + ": null pointer");
  for (int o = 0; o < m.B * m.P; ++o)
    GPK_REQUIRE(h, c.coord_of[o] >= 0 && c.coord_of[o] < c.nx && c.model_of[c.coord_of[o]] == o, name + ": outputs and coordinates disagree");
  SmallK k{};
  GPK_TRY(small_params(h, name, m, false, false, k));
  const int ps = hvp_slice((int)M, c.nx, m.P);
  hipLaunchKernelGGL(small_hvp_kernel, dim3(hess_groups(Np), m.B, (unsigned)((m.P + ps - 1) / ps)), dim3(256), 0, h->stream, k, c,
                     (long long)m.N, Np, m.D, m.P, Xq, (int)M, shares);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}
