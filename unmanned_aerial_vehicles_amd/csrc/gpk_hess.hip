// K8, second derivatives: the input Hessian of the posterior mean (fp64) - what an exact-Hessian SQP step, the second-order
// mean correction tr(H Sigma) / 2 and the state sensitivity of the linearisation need.
//
//   q = x* / ls, r_j = x_j / ls, delta_j = q - r_j (exact differences, formed before any product), k_j = sf2 exp(-|delta_j|^2 / 2)
//   T_p[d][e] = sum_j k_j alpha_jp delta_jd delta_je          (symmetric: D (D + 1) / 2 sums per (query, output))
//   S_p       = sum_j k_j alpha_jp
//   d2 mean_p / dx*_d dx*_e = y_std[p] / (ls_d ls_e) (T_p[d][e] - [d = e] S_p)
//
//   predict_mean_hess_kernel  the companion of predict_mean_grad_kernel (gpk_jac.hip), the same tiling: training rows staged
//                             through LDS already divided by ls_d, one query per thread, one exp per (query, training point)
//                             pair.  The lower triangle of T is cut into blocks of whole rows [R0, R1) so that a thread keeps at
//                             most 64 fp64 accumulators (no scratch): D <= 4 one block with up to 4 outputs, D <= 8 one block,
//                             D <= 12 two and D <= 16 three blocks with one output.  (output group, row block) is the third grid
//                             dimension; every such group recomputes the pair's kernel value, as the Jacobian's output groups
//                             do.  Row block 0 also carries S_p.  The training set is cut into chunks (second grid dimension).
//   mean_hess_reduce_kernel   adds the chunks in chunk order, subtracts S_p on the diagonal, applies y_std[p] sf2 / (ls_d ls_e)
//                             and writes H[d][e] and H[e][d] from the one sum: symmetric bit for bit, no floating-point atomics,
//                             bit-identical from run to run.
//   predict_mean_hess_multi_kernel  the companion of predict_mean_grad_multi_kernel for B <= 8 single-output ARD models on shared
//                             inputs (the per-axis batch): rows staged raw with the B alpha columns, the raw feature differences
//                             of a pair and each product of two of them formed ONCE and used by every model's distance (its
//                             1 / ls^2 weights in LDS) and every model's sums; the models in groups of two (D <= 4: up to four)
//                             and the triangle in row blocks of at most 31 entries over the third grid dimension (<= 62
//                             accumulators, no scratch); mean_hess_reduce_multi_kernel applies 1 / (ls_bd ls_be).
//
// No reference counterpart: scikit-learn has no derivative call.  A caller of the reference would difference
// GaussianProcessRegressor.predict (sklearn/gaussian_process/_gpr.py:441-494) twice; within this library, 2 D (fourth order:
// 4 D) gpk_predict_host_grad calls.
#include "gpk_internal.h"
#include "gpk_math.h"

namespace {

struct HLs16 { double v[16]; };
struct HP16 { double v[16]; };

constexpr int HS_TJ = 128;                      // training rows staged per round
constexpr int64_t HS_PANEL = 65536;             // queries per launch at the most
constexpr size_t HS_PARTIAL_BYTES = 256u << 20; // bound on the chunks' partial sums (S x panel x P x (D (D + 1) / 2 + 1) doubles)

constexpr int tri(int d) { return d * (d + 1) / 2; }      // packed index of the first entry of row d: (d, e <= d) at tri(d) + e

// partial[chunk][m][p][tri(d) + e] = sum_{j in chunk} exp(-|q_m - r_j|^2 / 2) alpha_jp delta_jd delta_je  for R0 <= d < R1, e <= d;
// partial[chunk][m][p][tri(D)]     = sum_{j in chunk} exp(-|q_m - r_j|^2 / 2) alpha_jp                    (row block 0)
template <int D4, int PS, int R0, int R1>
__device__ __forceinline__ void mean_hess_body(double* __restrict__ rows, const double* __restrict__ X,
                                               const double* __restrict__ alpha, long long N, int D, int P, const HLs16& ls,
                                               const double* __restrict__ Xq, long long M, long long chunk, int p0,
                                               double* __restrict__ partial) {
  constexpr int DD = 4 * D4, RS = DD + 4, NT = tri(R1) - tri(R0);
  static_assert((NT + 1) * PS <= 64, "at most 64 fp64 accumulators per thread");
  const int tid = threadIdx.x;
  const long long qm = (long long)blockIdx.x * 256 + tid;
  double xq[DD], acc[PS][NT], s0[PS];
#pragma unroll
  for (int d = 0; d < DD; ++d) {
    xq[d] = 0.0;
    if (d < D && qm < M) xq[d] = Xq[qm * D + d] / ls.v[d];
  }
#pragma unroll
  for (int p = 0; p < PS; ++p) {
    s0[p] = 0.0;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[p][t] = 0.0;
  }
  const long long n0 = (long long)blockIdx.y * chunk;
  const long long n1 = min(N, n0 + chunk);
  for (long long jb = n0; jb < n1; jb += HS_TJ) {
    const int nj = (int)min((long long)HS_TJ, n1 - jb);
    __syncthreads();
    // stage [x / ls | 0.. | alpha of this group's outputs | 0..] for the nj rows of this round
    for (int e = tid; e < nj * RS; e += 256) {
      const int j = e / RS, c = e - j * RS;
      double v = 0.0;
      if (c < DD) { if (c < D) v = X[(jb + j) * D + c] / ls.v[c]; }
      else if (c - DD < PS && p0 + (c - DD) < P) v = alpha[(jb + j) * P + p0 + (c - DD)];
      rows[e] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
      const double4* row = reinterpret_cast<const double4*>(rows + j * RS);
      double df[DD], al[4];
#pragma unroll
      for (int g = 0; g < D4; ++g) {
        const double4 v = row[g];
        df[4 * g] = xq[4 * g] - v.x; df[4 * g + 1] = xq[4 * g + 1] - v.y;
        df[4 * g + 2] = xq[4 * g + 2] - v.z; df[4 * g + 3] = xq[4 * g + 3] - v.w;
      }
      {
        const double4 v = row[D4];
        al[0] = v.x; al[1] = v.y; al[2] = v.z; al[3] = v.w;
      }
      double d2 = 0.0;
#pragma unroll
      for (int d = 0; d < DD; ++d) d2 = __builtin_fma(df[d], df[d], d2);
      const double ex = gpk_exp_neg(-0.5 * d2);
#pragma unroll
      for (int p = 0; p < PS; ++p) {
        const double w = ex * al[p];
        if (R0 == 0) s0[p] += w;
#pragma unroll
        for (int d = R0; d < R1; ++d) {
          const double wd = w * df[d];
#pragma unroll
          for (int e = 0; e <= d; ++e) acc[p][tri(d) - tri(R0) + e] = __builtin_fma(wd, df[e], acc[p][tri(d) - tri(R0) + e]);
        }
      }
    }
  }
  if (qm < M) {
    const int TP = tri(D) + 1;
#pragma unroll
    for (int p = 0; p < PS; ++p)
      if (p0 + p < P) {
        double* out = partial + (((long long)blockIdx.y * M + qm) * P + p0 + p) * TP;
#pragma unroll
        for (int d = R0; d < R1; ++d)
          if (d < D) {
#pragma unroll
            for (int e = 0; e <= d; ++e) out[tri(d) + e] = acc[p][tri(d) - tri(R0) + e];
          }
        if (R0 == 0) out[TP - 1] = s0[p];
      }
  }
}

// blockIdx.z = output group * (number of row blocks) + row block; the row blocks of D4: 1, 2: [0, DD); 3: [0, 8) [8, 12);
// 4: [0, 9) [9, 13) [13, 16) - 37 / 42 and 46 / 46 / 45 accumulators
template <int D4, int PS>
__global__ __launch_bounds__(256) void predict_mean_hess_kernel(const double* __restrict__ X, const double* __restrict__ alpha,
                                                                long long N, int D, int P, HLs16 ls,
                                                                const double* __restrict__ Xq, long long M, long long chunk,
                                                                double* __restrict__ partial) {
  constexpr int DD = 4 * D4, RS = DD + 4;
  __shared__ __attribute__((aligned(32))) double rows[HS_TJ * RS];
  if constexpr (D4 <= 2) {
    mean_hess_body<D4, PS, 0, DD>(rows, X, alpha, N, D, P, ls, Xq, M, chunk, (int)blockIdx.z * PS, partial);
  } else if constexpr (D4 == 3) {
    static_assert(PS == 1, "one output per group above D = 8");
    const int p0 = blockIdx.z >> 1;
    if ((blockIdx.z & 1) == 0) mean_hess_body<3, 1, 0, 8>(rows, X, alpha, N, D, P, ls, Xq, M, chunk, p0, partial);
    else mean_hess_body<3, 1, 8, 12>(rows, X, alpha, N, D, P, ls, Xq, M, chunk, p0, partial);
  } else {
    static_assert(PS == 1, "one output per group above D = 8");
    const int p0 = blockIdx.z / 3, rb = blockIdx.z - 3 * p0;
    if (rb == 0) mean_hess_body<4, 1, 0, 9>(rows, X, alpha, N, D, P, ls, Xq, M, chunk, p0, partial);
    else if (rb == 1) mean_hess_body<4, 1, 9, 13>(rows, X, alpha, N, D, P, ls, Xq, M, chunk, p0, partial);
    else mean_hess_body<4, 1, 13, 16>(rows, X, alpha, N, D, P, ls, Xq, M, chunk, p0, partial);
  }
}

// hess[m][p][d][e] = hess[m][p][e][d] = y_std[p] sf2 / (ls_d ls_e) (sum_chunks T[d][e] - [d = e] sum_chunks S); one thread per
// (m, p, d, e <= d), the chunks in order
__global__ void mean_hess_reduce_kernel(const double* __restrict__ partial, int S, long long M, int D, int P, double sf2, HLs16 ls,
                                        HP16 ystd, double* __restrict__ hess) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int TT = tri(D), TP = TT + 1;
  if (i >= M * P * TT) return;
  const int t = (int)(i % TT);
  const long long mp = i / TT;
  const int p = (int)(mp % P);
  int d = 0;
  while (tri(d + 1) <= t) ++d;
  const int e = t - tri(d);
  const long long stride = M * P * TP;
  const double* src = partial + mp * TP;
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += src[(long long)k * stride + t];
  if (d == e) {
    double s0 = 0.0;
    for (int k = 0; k < S; ++k) s0 += src[(long long)k * stride + TT];
    s -= s0;
  }
  const double v = (ystd.v[p] * sf2 / (ls.v[d] * ls.v[e])) * s;
  double* out = hess + mp * D * D;
  out[d * D + e] = v;
  out[e * D + d] = v;
}

// ---- mean Hessian of B single-output models on shared inputs ------------------------------------------------------------
struct HW128 { double v[8 * 16]; };      // [model][feature]

// partial[chunk][m][b][tri(d) + e] = sum_{j in chunk} exp(-sum_d' (x_jd' - q_md')^2 w_bd' / 2) alpha_jb (x_jd - q_md) (x_je - q_me),
// w_bd = 1 / ls_bd^2, for R0 <= d < R1, e <= d;  partial[chunk][m][b][tri(D)] = the same sum without the two differences (block 0).
// The raw differences of a pair and each product of two of them are formed ONCE and serve every model of the group.
template <int D4, int BS, int R0, int R1>
__device__ __forceinline__ void mean_hess_multi_body(double* __restrict__ rows, const double* __restrict__ wl,
                                                     const double* __restrict__ X, const double* __restrict__ alpha, long long N,
                                                     int D, int B, const double* __restrict__ Xq, long long M, long long chunk,
                                                     int b0, double* __restrict__ partial) {
  constexpr int DD = 4 * D4, RS = DD + 4, NT = tri(R1) - tri(R0);
  static_assert((NT + (R0 == 0 ? 1 : 0)) * BS <= 64, "at most 64 fp64 accumulators per thread");
  const int tid = threadIdx.x;
  const long long qm = (long long)blockIdx.x * 256 + tid;
  double xq[DD], acc[BS][NT], s0[BS];
#pragma unroll
  for (int d = 0; d < DD; ++d) {
    xq[d] = 0.0;
    if (d < D && qm < M) xq[d] = Xq[qm * D + d];
  }
#pragma unroll
  for (int b = 0; b < BS; ++b) {
    s0[b] = 0.0;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[b][t] = 0.0;
  }
  const long long n0 = (long long)blockIdx.y * chunk;
  const long long n1 = min(N, n0 + chunk);
  for (long long jb = n0; jb < n1; jb += HS_TJ) {
    const int nj = (int)min((long long)HS_TJ, n1 - jb);
    __syncthreads();
    // stage [x | 0.. | alpha of this group's models | 0..] for the nj rows of this round
    for (int e = tid; e < nj * RS; e += 256) {
      const int j = e / RS, c = e - j * RS;
      double v = 0.0;
      if (c < DD) { if (c < D) v = X[(jb + j) * D + c]; }
      else if (c - DD < BS && b0 + (c - DD) < B) v = alpha[(jb + j) * B + b0 + (c - DD)];
      rows[e] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
      const double4* row = reinterpret_cast<const double4*>(rows + j * RS);
      double df[DD], al[4], w[BS];
#pragma unroll
      for (int g = 0; g < D4; ++g) {
        const double4 v = row[g];
        df[4 * g] = v.x - xq[4 * g]; df[4 * g + 1] = v.y - xq[4 * g + 1];
        df[4 * g + 2] = v.z - xq[4 * g + 2]; df[4 * g + 3] = v.w - xq[4 * g + 3];
      }
      {
        const double4 v = row[D4];
        al[0] = v.x; al[1] = v.y; al[2] = v.z; al[3] = v.w;
      }
#pragma unroll
      for (int b = 0; b < BS; ++b) {
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < DD; ++d) d2 = __builtin_fma(df[d] * df[d], wl[b * DD + d], d2);
        w[b] = gpk_exp_neg(-0.5 * d2) * al[b];
        if (R0 == 0) s0[b] += w[b];
      }
#pragma unroll
      for (int d = R0; d < R1; ++d) {
#pragma unroll
        for (int e = 0; e <= d; ++e) {
          const double pr = df[d] * df[e];
#pragma unroll
          for (int b = 0; b < BS; ++b) acc[b][tri(d) - tri(R0) + e] = __builtin_fma(w[b], pr, acc[b][tri(d) - tri(R0) + e]);
        }
      }
    }
  }
  if (qm < M) {
    const int TP = tri(D) + 1;
#pragma unroll
    for (int b = 0; b < BS; ++b)
      if (b0 + b < B) {
        double* out = partial + (((long long)blockIdx.y * M + qm) * B + b0 + b) * TP;
#pragma unroll
        for (int d = R0; d < R1; ++d)
          if (d < D) {
#pragma unroll
            for (int e = 0; e <= d; ++e) out[tri(d) + e] = acc[b][tri(d) - tri(R0) + e];
          }
        if (R0 == 0) out[TP - 1] = s0[b];
      }
  }
}

// blockIdx.z = model group * (number of row blocks) + row block.  D <= 4: groups of BS <= 4 models, one block; above: groups of
// two models and row blocks of at most 31 entries: D4 = 2: [0, 5) [5, 8); 3: [0, 7) [7, 10) [10, 12); 4: those and [12, 14)
// [14, 16) - at most 62 accumulators
template <int D4, int BS>
__global__ __launch_bounds__(256) void predict_mean_hess_multi_kernel(const double* __restrict__ X, const double* __restrict__ alpha,
                                                                      long long N, int D, int B, HW128 wt,
                                                                      const double* __restrict__ Xq, long long M, long long chunk,
                                                                      double* __restrict__ partial) {
  constexpr int DD = 4 * D4, RS = DD + 4, NRB = D4 == 1 ? 1 : D4 == 2 ? 2 : D4 == 3 ? 3 : 5;
  __shared__ __attribute__((aligned(32))) double rows[HS_TJ * RS];
  __shared__ double wl[BS * DD];          // this group's weights (0 in the padding)
  const int g = blockIdx.z / NRB, rb = blockIdx.z - g * NRB, b0 = g * BS;
  for (int e = threadIdx.x; e < BS * DD; e += 256) {
    const int b = e / DD, d = e - b * DD;
    wl[e] = (b0 + b < B && d < D) ? wt.v[(b0 + b) * 16 + d] : 0.0;
  }
  // (the body's first staging round starts with a barrier: wl is complete before anyone reads it)
  if constexpr (D4 == 1) {
    mean_hess_multi_body<1, BS, 0, 4>(rows, wl, X, alpha, N, D, B, Xq, M, chunk, b0, partial);
  } else if constexpr (D4 == 2) {
    if (rb == 0) mean_hess_multi_body<2, BS, 0, 5>(rows, wl, X, alpha, N, D, B, Xq, M, chunk, b0, partial);
    else mean_hess_multi_body<2, BS, 5, 8>(rows, wl, X, alpha, N, D, B, Xq, M, chunk, b0, partial);
  } else {
    if (rb == 0) mean_hess_multi_body<D4, BS, 0, 7>(rows, wl, X, alpha, N, D, B, Xq, M, chunk, b0, partial);
    else if (rb == 1) mean_hess_multi_body<D4, BS, 7, 10>(rows, wl, X, alpha, N, D, B, Xq, M, chunk, b0, partial);
    else if (rb == 2) mean_hess_multi_body<D4, BS, 10, 12>(rows, wl, X, alpha, N, D, B, Xq, M, chunk, b0, partial);
    else if constexpr (D4 == 4) {
      if (rb == 3) mean_hess_multi_body<4, BS, 12, 14>(rows, wl, X, alpha, N, D, B, Xq, M, chunk, b0, partial);
      else mean_hess_multi_body<4, BS, 14, 16>(rows, wl, X, alpha, N, D, B, Xq, M, chunk, b0, partial);
    }
  }
}

// hess[m][b][d][e] = hess[m][b][e][d] = c_b g (g sum_chunks T_raw[d][e] - [d = e] sum_chunks S), g = 1 / (ls_bd ls_be),
// c_b = y_std[b] sf2[b] (il: [model][feature] = 1 / ls_bd); one thread per (m, b, d, e <= d), the chunks in order
__global__ void mean_hess_reduce_multi_kernel(const double* __restrict__ partial, int S, long long M, int D, int B, HW128 il,
                                              HP16 c, double* __restrict__ hess) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int TT = tri(D), TP = TT + 1;
  if (i >= M * B * TT) return;
  const int t = (int)(i % TT);
  const long long mb = i / TT;
  const int b = (int)(mb % B);
  int d = 0;
  while (tri(d + 1) <= t) ++d;
  const int e = t - tri(d);
  const long long stride = M * B * TP;
  const double* src = partial + mb * TP;
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += src[(long long)k * stride + t];
  const double g = il.v[b * 16 + d] * il.v[b * 16 + e];
  s *= g;
  if (d == e) {
    double s0 = 0.0;
    for (int k = 0; k < S; ++k) s0 += src[(long long)k * stride + TT];
    s -= s0;
  }
  const double v = (c.v[b] * g) * s;
  double* out = hess + mb * D * D;
  out[d * D + e] = v;
  out[e * D + d] = v;
}

using mhm_fn = void (*)(const double*, const double*, long long, int, int, HW128, const double*, long long, long long, double*);
mhm_fn mhm_pick(int d4, int bs) {
  switch (d4) {
    case 1:
      switch (bs) {
        case 1: return predict_mean_hess_multi_kernel<1, 1>;
        case 2: return predict_mean_hess_multi_kernel<1, 2>;
        case 3: return predict_mean_hess_multi_kernel<1, 3>;
        default: return predict_mean_hess_multi_kernel<1, 4>;
      }
    case 2: return predict_mean_hess_multi_kernel<2, 2>;
    case 3: return predict_mean_hess_multi_kernel<3, 2>;
    default: return predict_mean_hess_multi_kernel<4, 2>;
  }
}

using mh_fn = void (*)(const double*, const double*, long long, int, int, HLs16, const double*, long long, long long, double*);
mh_fn mh_pick(int d4, int ps) {
  switch (d4) {
    case 1:
      switch (ps) {
        case 1: return predict_mean_hess_kernel<1, 1>;
        case 2: return predict_mean_hess_kernel<1, 2>;
        case 3: return predict_mean_hess_kernel<1, 3>;
        default: return predict_mean_hess_kernel<1, 4>;
      }
    case 2: return predict_mean_hess_kernel<2, 1>;
    case 3: return predict_mean_hess_kernel<3, 1>;
    default: return predict_mean_hess_kernel<4, 1>;
  }
}

}  // namespace

extern "C" int gpk_predict_mean_hess(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P,
                                     const double* ls, double sf2, const double* y_std, const double* Xq, int64_t M,
                                     double* hess) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, hess != nullptr, "predict_mean_hess: hess is null");
  GPK_REQUIRE(h, X && alpha && Xq && y_std && ls, "predict_mean_hess: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1, "predict_mean_hess: empty input");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT, "predict_mean_hess: D must be in [1, 16]");
  GPK_REQUIRE(h, P >= 1 && P <= GPK_MAX_P, "predict_mean_hess: P must be in [1, 16]");
  HLs16 l;
  for (int d = 0; d < 16; ++d) l.v[d] = 1.0;
  for (int d = 0; d < D; ++d) {
    GPK_REQUIRE(h, ls[d] > 0.0, "predict_mean_hess: length-scales must be positive");
    l.v[d] = ls[d];
  }
  HP16 ys{};
  for (int p = 0; p < P; ++p) ys.v[p] = y_std[p];
  const int d4 = (D + 3) / 4;
  // D <= 4: output groups of PS <= 4, the fewest groups, evenly filled (as gpk_predict_mean_grad); above: one output per group
  const int npg = d4 == 1 ? (P + 3) / 4 : P, ps = d4 == 1 ? (P + npg - 1) / npg : 1;
  const int nrb = d4 <= 2 ? 1 : d4 - 1;
  const int64_t TP = (int64_t)tri(D) + 1;
  // query panels whose partial sums fit the bound with one chunk at least
  int64_t panel = (int64_t)(HS_PARTIAL_BYTES / ((size_t)P * TP * sizeof(double))) / 256 * 256;
  if (panel > HS_PANEL) panel = HS_PANEL;
  if (panel < 256) panel = 256;
  for (int64_t m0 = 0; m0 < M; m0 += panel) {
    const int64_t mc = M - m0 < panel ? M - m0 : panel;
    const int64_t nqb = (mc + 255) / 256;
    // the chunking of gpk_predict_mean_grad (~2048 workgroups; 32-row granularity for the control loop's sizes), then as few
    // chunks as keep the partial sums within HS_PARTIAL_BYTES
    const int64_t gran = (mc <= 512 && N <= 16384) ? 32 : HS_TJ;
    const int64_t nz = (int64_t)npg * nrb;
    int64_t S = (2048 + nqb * nz - 1) / (nqb * nz);
    const int64_t maxS = (N + gran - 1) / gran;
    const int64_t capS = (int64_t)(HS_PARTIAL_BYTES / ((size_t)mc * P * TP * sizeof(double)));
    if (S > capS) S = capS;
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    if (S > 65535) S = 65535;
    int64_t chunk = (N + S - 1) / S;
    chunk = (chunk + gran - 1) / gran * gran;
    S = (N + chunk - 1) / chunk;
    if (h->gram_log)   // option gram_log = 1: the form this launch pair takes (the tests assert it per case)
      fprintf(stderr, "GPKDERIV mean_hess %lld %d %d %lld d4%d ps%d ng%d nrb%d nqb%lld gran%lld s%lld chunk%lld\n", (long long)N, D, P,
              (long long)mc, d4, ps, npg, nrb, (long long)nqb, (long long)gran, (long long)S, (long long)chunk);
    void* partial = nullptr;
    GPK_TRY(gpk_scratch(h, (size_t)S * mc * P * TP * sizeof(double), &partial));
    hipLaunchKernelGGL(mh_pick(d4, ps), dim3((unsigned)nqb, (unsigned)S, (unsigned)nz), dim3(256), 0, h->stream, X, alpha,
                       (long long)N, D, P, l, Xq + m0 * D, (long long)mc, (long long)chunk, (double*)partial);
    GPK_LAUNCH_CHECK(h);
    const int64_t tot = mc * P * tri(D);
    hipLaunchKernelGGL(mean_hess_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)partial, (int)S, (long long)mc, D, P, sf2, l, ys, hess + m0 * P * D * D);
    GPK_LAUNCH_CHECK(h);
  }
  return GPK_OK;
}

extern "C" int gpk_predict_mean_hess_multi(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int B,
                                           const double* ls, const double* sf2, const double* y_std, const double* Xq, int64_t M,
                                           double* hess) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, hess != nullptr, "predict_mean_hess_multi: hess is null");
  GPK_REQUIRE(h, X && alpha && Xq && ls && sf2 && y_std, "predict_mean_hess_multi: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1, "predict_mean_hess_multi: empty input");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT, "predict_mean_hess_multi: D must be in [1, 16]");
  GPK_REQUIRE(h, B >= 1 && B <= 8, "predict_mean_hess_multi: B must be in [1, 8]");
  HW128 wt{}, il{};
  HP16 c{};
  for (int b = 0; b < B; ++b) {
    c.v[b] = y_std[b] * sf2[b];
    for (int d = 0; d < D; ++d) {
      const double l = ls[b * D + d];
      GPK_REQUIRE(h, l > 0.0, "predict_mean_hess_multi: length-scales must be positive");
      wt.v[b * 16 + d] = 1.0 / (l * l);
      il.v[b * 16 + d] = 1.0 / l;
    }
  }
  const int d4 = (D + 3) / 4;
  // D <= 4: model groups of BS <= 4, the fewest groups, evenly filled (as gpk_predict_mean_grad_multi); above: groups of two
  const int ng = d4 == 1 ? (B + 3) / 4 : (B + 1) / 2, bs = d4 == 1 ? (B + ng - 1) / ng : 2;
  const int nrb = d4 == 1 ? 1 : d4 == 2 ? 2 : d4 == 3 ? 3 : 5;
  const int64_t TP = (int64_t)tri(D) + 1;
  int64_t panel = (int64_t)(HS_PARTIAL_BYTES / ((size_t)B * TP * sizeof(double))) / 256 * 256;
  if (panel > HS_PANEL) panel = HS_PANEL;
  if (panel < 256) panel = 256;
  for (int64_t m0 = 0; m0 < M; m0 += panel) {
    const int64_t mc = M - m0 < panel ? M - m0 : panel;
    const int64_t nqb = (mc + 255) / 256;
    // the chunking of gpk_predict_mean_hess
    const int64_t gran = (mc <= 512 && N <= 16384) ? 32 : HS_TJ;
    const int64_t nz = (int64_t)ng * nrb;
    int64_t S = (2048 + nqb * nz - 1) / (nqb * nz);
    const int64_t maxS = (N + gran - 1) / gran;
    const int64_t capS = (int64_t)(HS_PARTIAL_BYTES / ((size_t)mc * B * TP * sizeof(double)));
    if (S > capS) S = capS;
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    if (S > 65535) S = 65535;
    int64_t chunk = (N + S - 1) / S;
    chunk = (chunk + gran - 1) / gran * gran;
    S = (N + chunk - 1) / chunk;
    if (h->gram_log)
      fprintf(stderr, "GPKDERIV mean_hess_multi %lld %d %d %lld d4%d bs%d ng%d nrb%d nqb%lld gran%lld s%lld chunk%lld\n", (long long)N, D,
              B, (long long)mc, d4, bs, ng, nrb, (long long)nqb, (long long)gran, (long long)S, (long long)chunk);
    void* partial = nullptr;
    GPK_TRY(gpk_scratch(h, (size_t)S * mc * B * TP * sizeof(double), &partial));
    hipLaunchKernelGGL(mhm_pick(d4, bs), dim3((unsigned)nqb, (unsigned)S, (unsigned)nz), dim3(256), 0, h->stream, X, alpha,
                       (long long)N, D, B, wt, Xq + m0 * D, (long long)mc, (long long)chunk, (double*)partial);
    GPK_LAUNCH_CHECK(h);
    const int64_t tot = mc * B * tri(D);
    hipLaunchKernelGGL(mean_hess_reduce_multi_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)partial, (int)S, (long long)mc, D, B, il, c, hess + m0 * B * D * D);
    GPK_LAUNCH_CHECK(h);
  }
  return GPK_OK;
}
