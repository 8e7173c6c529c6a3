// K8: input gradients of the posterior (fp64) - the first-order terms a model-predictive controller linearises with:
//
//   u_jd            = (x_jd - x*_d) / ls_d^2                             (exact differences, as everywhere)
//   d mean_p / dx*_d =  y_std[p] sum_j k(x*, x_j) u_jd alpha_jp
//   d var    / dx*_d = -2 sum_j k(x*, x_j) u_jd c_j,   c = K^-1 k* = W^T (W k*)      (normalised-target units)
//
//   predict_mean_grad_kernel  the tiling of predict_mean_kernel (gpk_gram.hip): training rows staged through LDS already
//                             divided by ls_d, one query per thread, one exp per (query, training point) pair; the pair
//                             contributes k alpha_jp (x*_d - x_jd) / ls_d to D x PS running sums.  D x P can reach 256
//                             accumulators per query, so the outputs are split into groups of PS <= 4 over the third grid
//                             dimension (at most 64 accumulators = 128 VGPRs per thread, no scratch); a group recomputes the
//                             pair's kernel value (D subtract / FMA pairs and one exp against the group's D x PS FMAs).  The
//                             training set is cut into chunks (second grid dimension) whose partial sums mean_grad_reduce_kernel
//                             adds in chunk order: bit-identical from run to run.  The N x M x D tensor of kernel derivatives is
//                             never stored.
//   var_grad_kernel           after K* (gpk_cross_gram_t, training-major), V = W K* and C = W^T V (two tile GEMMs, W's zero
//                             triangle skipped in both): ONE streaming pass over the three Np x Mp panels, one query column per
//                             thread: sum_j K*[j][m] C[j][m] (x_jd - x*_d) / ls_d for every d and sum_j V[j][m]^2, per chunk of
//                             training rows; var_grad_finalize_kernel adds the chunks in order and writes
//                             dvar = -2 / ls_d * sum and var = max(kss - sum V^2, floor).
//
//   predict_mean_grad_multi_kernel  the Jacobian companion of predict_mean_multi_kernel (gpk_gram.hip) for B <= 8 single-output
//                             ARD models on shared inputs (the per-axis batch): rows staged raw with the B alpha columns, the raw
//                             feature differences of a pair formed ONCE and used by every model's distance (its 1 / ls^2 weights
//                             in LDS) and every model's D running sums; the models in groups of <= 4 over the third grid
//                             dimension (<= 64 accumulators, no scratch), the training set in chunks added in chunk order.
//
// No reference counterpart: scikit-learn has no gradient call.  A caller of the reference would difference
// GaussianProcessRegressor.predict (sklearn/gaussian_process/_gpr.py:441-494) around the horizon loop of
// src/px4/mpc.py:1490-1506; the consumer is the linearisation of quadrotor_gp_mpc/quadrotor_gp_mpc/mpc_controller.py:318.
#include "gpk_internal.h"
#include "gpk_math.h"

namespace {

struct Ls16 { double v[16]; };
struct P16 { double v[16]; };

constexpr int JG_TJ = 128;       // training rows staged per round

// ---- mean Jacobian -----------------------------------------------------------------------------------------------------
// partial[chunk][m][p][d] = sum_{j in chunk} exp(-|q_m - x_j|^2 / 2) alpha_jp (q_md - x_jd)   (q, x divided by ls)
template <int D4, int PS>
__global__ __launch_bounds__(256) void predict_mean_grad_kernel(const double* __restrict__ X, const double* __restrict__ alpha,
                                                                long long N, int D, int P, Ls16 ls,
                                                                const double* __restrict__ Xq, long long M, long long chunk,
                                                                double* __restrict__ partial) {
  constexpr int DD = 4 * D4, RS = DD + 4;
  __shared__ __attribute__((aligned(32))) double rows[JG_TJ * RS];
  const int tid = threadIdx.x;
  const int p0 = blockIdx.z * PS;
  const long long qm = (long long)blockIdx.x * 256 + tid;
  double xq[DD], acc[DD][PS];
#pragma unroll
  for (int d = 0; d < DD; ++d) {
    xq[d] = 0.0;
    if (d < D && qm < M) xq[d] = Xq[qm * D + d] / ls.v[d];
#pragma unroll
    for (int p = 0; p < PS; ++p) acc[d][p] = 0.0;
  }
  const long long n0 = (long long)blockIdx.y * chunk;
  const long long n1 = min(N, n0 + chunk);
  for (long long jb = n0; jb < n1; jb += JG_TJ) {
    const int nj = (int)min((long long)JG_TJ, n1 - jb);
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
#pragma unroll 2
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
      const double e = gpk_exp_neg(-0.5 * d2);
#pragma unroll
      for (int p = 0; p < PS; ++p) {
        const double w = e * al[p];
#pragma unroll
        for (int d = 0; d < DD; ++d) acc[d][p] = __builtin_fma(w, df[d], acc[d][p]);
      }
    }
  }
  if (qm < M) {
#pragma unroll
    for (int p = 0; p < PS; ++p)
      if (p0 + p < P) {
        double* out = partial + (((long long)blockIdx.y * M + qm) * P + p0 + p) * D;
#pragma unroll
        for (int d = 0; d < DD; ++d)
          if (d < D) out[d] = acc[d][p];
      }
  }
}

// dmean[m][p][d] = -y_std[p] sf2 / ls_d * sum_chunks partial   (the staged difference is q - x: u = -(q - x) / ls)
__global__ void mean_grad_reduce_kernel(const double* __restrict__ partial, int S, long long M, int D, int P, double sf2, Ls16 ls,
                                        P16 ystd, double* __restrict__ dmean) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long tot = M * P * D;
  if (e >= tot) return;
  const int d = (int)(e % D), p = (int)((e / D) % P);
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += partial[(long long)k * tot + e];
  dmean[e] = -(ystd.v[p] * sf2 / ls.v[d]) * s;
}

// ---- mean Jacobian of B single-output models on shared inputs ---------------------------------------------------------
struct W128 { double v[8 * 16]; };      // [model][feature]

// partial[chunk][m][b][d] = sum_{j in chunk} exp(-sum_d' (x_jd' - q_md')^2 w_bd' / 2) alpha_jb (x_jd - q_md),  w_bd = 1 / ls_bd^2
template <int D4, int BS>
__global__ __launch_bounds__(256) void predict_mean_grad_multi_kernel(const double* __restrict__ X,
                                                                      const double* __restrict__ alpha, long long N, int D, int B,
                                                                      W128 wt, const double* __restrict__ Xq, long long M,
                                                                      long long chunk, double* __restrict__ partial) {
  constexpr int DD = 4 * D4, RS = DD + 4;
  __shared__ __attribute__((aligned(32))) double rows[JG_TJ * RS];
  __shared__ double wl[BS * DD];          // this group's weights (0 in the padding)
  const int tid = threadIdx.x;
  const int b0 = blockIdx.z * BS;
  for (int e = tid; e < BS * DD; e += 256) {
    const int b = e / DD, d = e - b * DD;
    wl[e] = (b0 + b < B && d < D) ? wt.v[(b0 + b) * 16 + d] : 0.0;
  }
  const long long qm = (long long)blockIdx.x * 256 + tid;
  double xq[DD], acc[BS][DD];
#pragma unroll
  for (int d = 0; d < DD; ++d) {
    xq[d] = 0.0;
    if (d < D && qm < M) xq[d] = Xq[qm * D + d];
#pragma unroll
    for (int b = 0; b < BS; ++b) acc[b][d] = 0.0;
  }
  const long long n0 = (long long)blockIdx.y * chunk;
  const long long n1 = min(N, n0 + chunk);
  for (long long jb = n0; jb < n1; jb += JG_TJ) {
    const int nj = (int)min((long long)JG_TJ, n1 - jb);
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
    // (one row at a time: two in flight spill at D4 = BS = 4)
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
      const double4* row = reinterpret_cast<const double4*>(rows + j * RS);
      double df[DD], al[4];
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
        const double w = gpk_exp_neg(-0.5 * d2) * al[b];
#pragma unroll
        for (int d = 0; d < DD; ++d) acc[b][d] = __builtin_fma(w, df[d], acc[b][d]);
      }
    }
  }
  if (qm < M) {
#pragma unroll
    for (int b = 0; b < BS; ++b)
      if (b0 + b < B) {
        double* out = partial + (((long long)blockIdx.y * M + qm) * B + b0 + b) * D;
#pragma unroll
        for (int d = 0; d < DD; ++d)
          if (d < D) out[d] = acc[b][d];
      }
  }
}

// dmean[m][b][d] = y_std[b] sf2[b] / ls_bd^2 * sum_chunks partial  (scale: [model][feature]); the chunks in order
__global__ void mean_grad_reduce_multi_kernel(const double* __restrict__ partial, int S, long long M, int D, int B, W128 scale,
                                              double* __restrict__ dmean) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long tot = M * B * D;
  if (e >= tot) return;
  const int d = (int)(e % D), b = (int)((e / D) % B);
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += partial[(long long)k * tot + e];
  dmean[e] = scale.v[b * 16 + d] * s;
}

using mgm_fn = void (*)(const double*, const double*, long long, int, int, W128, const double*, long long, long long, double*);
template <int D4>
mgm_fn mgm_pick_b(int bs) {
  switch (bs) {
    case 1: return predict_mean_grad_multi_kernel<D4, 1>;
    case 2: return predict_mean_grad_multi_kernel<D4, 2>;
    case 3: return predict_mean_grad_multi_kernel<D4, 3>;
    default: return predict_mean_grad_multi_kernel<D4, 4>;
  }
}
mgm_fn mgm_pick(int d4, int bs) {
  switch (d4) {
    case 1: return mgm_pick_b<1>(bs);
    case 2: return mgm_pick_b<2>(bs);
    case 3: return mgm_pick_b<3>(bs);
    default: return mgm_pick_b<4>(bs);
  }
}

using mg_fn = void (*)(const double*, const double*, long long, int, int, Ls16, const double*, long long, long long, double*);
template <int D4>
mg_fn mg_pick_p(int ps) {
  switch (ps) {
    case 1: return predict_mean_grad_kernel<D4, 1>;
    case 2: return predict_mean_grad_kernel<D4, 2>;
    case 3: return predict_mean_grad_kernel<D4, 3>;
    default: return predict_mean_grad_kernel<D4, 4>;
  }
}
mg_fn mg_pick(int d4, int ps) {
  switch (d4) {
    case 1: return mg_pick_p<1>(ps);
    case 2: return mg_pick_p<2>(ps);
    case 3: return mg_pick_p<3>(ps);
    default: return mg_pick_p<4>(ps);
  }
}

// ---- variance gradient: the streaming pass over K*, C = K^-1 K* and V = W K* (all Np x ld, training-major) ----------------
constexpr int VG_TJ = 64;        // training rows staged per round
constexpr int VG_COLS = 128;     // query columns per workgroup (one per thread)

// pg[chunk][m][0..D) = sum_{j in chunk} K*[j][m] C[j][m] (x_jd - q_md)  (x, q divided by ls);  pg[chunk][m][D] = sum_j V[j][m]^2
template <int D4>
__global__ __launch_bounds__(VG_COLS) void var_grad_kernel(const double* __restrict__ X, long long N, int D, Ls16 ls,
                                                           const double* __restrict__ Xq, long long M,
                                                           const double* __restrict__ Kt, const double* __restrict__ Cm,
                                                           const double* __restrict__ V, long long ld, long long chunk,
                                                           double* __restrict__ pg) {
  constexpr int DD = 4 * D4;
  __shared__ __attribute__((aligned(32))) double xs[VG_TJ * DD];
  const int tid = threadIdx.x;
  const long long m = (long long)blockIdx.x * VG_COLS + tid;
  const bool live = m < M;
  double xq[DD], acc[DD], ss = 0.0;
#pragma unroll
  for (int d = 0; d < DD; ++d) {
    xq[d] = (d < D && live) ? Xq[m * D + d] / ls.v[d] : 0.0;
    acc[d] = 0.0;
  }
  const long long n0 = (long long)blockIdx.y * chunk;
  const long long n1 = min(N, n0 + chunk);
  const long long col = live ? m : 0;            // (columns >= M of the padded panels: read column 0, result dropped)
  for (long long jb = n0; jb < n1; jb += VG_TJ) {
    const int nj = (int)min((long long)VG_TJ, n1 - jb);
    __syncthreads();
    for (int e = tid; e < nj * DD; e += VG_COLS) {
      const int j = e / DD, c = e - j * DD;
      xs[e] = c < D ? X[(jb + j) * D + c] / ls.v[c] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < nj; ++j) {
      const long long o = (jb + j) * ld + col;
      const double kv = Kt[o], cv = Cm[o], vv = V[o];
      const double w = kv * cv;
      ss = __builtin_fma(vv, vv, ss);
      const double4* row = reinterpret_cast<const double4*>(xs + j * DD);
#pragma unroll
      for (int g = 0; g < D4; ++g) {
        const double4 x = row[g];
        acc[4 * g] = __builtin_fma(w, x.x - xq[4 * g], acc[4 * g]);
        acc[4 * g + 1] = __builtin_fma(w, x.y - xq[4 * g + 1], acc[4 * g + 1]);
        acc[4 * g + 2] = __builtin_fma(w, x.z - xq[4 * g + 2], acc[4 * g + 2]);
        acc[4 * g + 3] = __builtin_fma(w, x.w - xq[4 * g + 3], acc[4 * g + 3]);
      }
    }
  }
  if (live) {
    double* out = pg + ((long long)blockIdx.y * M + m) * (D + 1);
#pragma unroll
    for (int d = 0; d < DD; ++d)
      if (d < D) out[d] = acc[d];
    out[D] = ss;
  }
}

// dvar[m][d] = -2 / ls_d * sum_chunks, var[m] = max(kss - sum_chunks, floor); the chunks in order
__global__ void var_grad_finalize_kernel(const double* __restrict__ pg, int S, long long M, int D, Ls16 ls, double kss,
                                         double floor_, double* __restrict__ var, double* __restrict__ dvar) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long tot = M * (D + 1);
  if (e >= tot) return;
  const long long m = e / (D + 1);
  const int d = (int)(e - m * (D + 1));
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += pg[(long long)k * tot + e];
  if (d < D) dvar[m * D + d] = -2.0 / ls.v[d] * s;
  else if (var) var[m] = fmax(kss - s, floor_);
}

using vg_fn = void (*)(const double*, long long, int, Ls16, const double*, long long, const double*, const double*, const double*,
                       long long, long long, double*);
vg_fn vg_pick(int d4) {
  switch (d4) {
    case 1: return var_grad_kernel<1>;
    case 2: return var_grad_kernel<2>;
    case 3: return var_grad_kernel<3>;
    default: return var_grad_kernel<4>;
  }
}

int fill_ls16(gpk_handle h, const double* ls, int D, Ls16& out) {
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT, "D must be in [1, 16]");
  GPK_REQUIRE(h, ls != nullptr, "length-scale array is null");
  for (int d = 0; d < 16; ++d) out.v[d] = 1.0;
  for (int d = 0; d < D; ++d) {
    GPK_REQUIRE(h, ls[d] > 0.0, "length-scales must be positive");
    out.v[d] = ls[d];
  }
  return GPK_OK;
}

constexpr int64_t MG_PANEL = 65536;      // queries per launch of the mean Jacobian (bounds the partial sums' scratch)

}  // namespace

extern "C" int gpk_predict_mean_grad(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P,
                                     const double* ls, double sf2, const double* y_std, const double* Xq, int64_t M,
                                     double* dmean) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && Xq && dmean && y_std, "predict_mean_grad: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1, "predict_mean_grad: empty input");
  GPK_REQUIRE(h, P >= 1 && P <= GPK_MAX_P, "predict_mean_grad: P must be in [1, 16]");
  Ls16 l;
  GPK_TRY(fill_ls16(h, ls, D, l));
  P16 ys{};
  for (int p = 0; p < P; ++p) ys.v[p] = y_std[p];
  // output groups of PS <= 4: the fewest groups, evenly filled (P = 6: two groups of 3)
  const int npg = (P + 3) / 4, ps = (P + npg - 1) / npg, d4 = (D + 3) / 4;
  for (int64_t m0 = 0; m0 < M; m0 += MG_PANEL) {
    const int64_t mc = M - m0 < MG_PANEL ? M - m0 : MG_PANEL;
    const int64_t nqb = (mc + 255) / 256;
    // chunks of the training set so that the grid has ~2048 workgroups; a handful of queries against a small training set
    // (the control loop) is pure latency, so those get chunks of 32 rows (as gpk_predict_mean)
    const int64_t gran = (mc <= 512 && N <= 16384) ? 32 : JG_TJ;
    int64_t S = (2048 + nqb * npg - 1) / (nqb * npg);
    const int64_t maxS = (N + gran - 1) / gran;
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    if (S > 65535) S = 65535;
    int64_t chunk = (N + S - 1) / S;
    chunk = (chunk + gran - 1) / gran * gran;
    S = (N + chunk - 1) / chunk;
    if (h->gram_log)   // option gram_log = 1: the form this launch pair takes (the tests assert it per case)
      fprintf(stderr, "GPKDERIV mean_grad %lld %d %d %lld d4%d ps%d ng%d nrb1 nqb%lld gran%lld s%lld chunk%lld\n", (long long)N, D, P,
              (long long)mc, d4, ps, npg, (long long)nqb, (long long)gran, (long long)S, (long long)chunk);
    void* partial = nullptr;
    GPK_TRY(gpk_scratch(h, (size_t)S * mc * P * D * sizeof(double), &partial));
    hipLaunchKernelGGL(mg_pick(d4, ps), dim3((unsigned)nqb, (unsigned)S, (unsigned)npg), dim3(256), 0, h->stream, X, alpha,
                       (long long)N, D, P, l, Xq + m0 * D, (long long)mc, (long long)chunk, (double*)partial);
    GPK_LAUNCH_CHECK(h);
    const int64_t tot = mc * P * D;
    hipLaunchKernelGGL(mean_grad_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)partial, (int)S, (long long)mc, D, P, sf2, l, ys, dmean + m0 * P * D);
    GPK_LAUNCH_CHECK(h);
  }
  return GPK_OK;
}

extern "C" int gpk_predict_mean_grad_multi(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int B,
                                           const double* ls, const double* sf2, const double* y_std, const double* Xq, int64_t M,
                                           double* dmean) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && Xq && dmean && ls && sf2 && y_std, "predict_mean_grad_multi: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1, "predict_mean_grad_multi: empty input");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT, "predict_mean_grad_multi: D must be in [1, 16]");
  GPK_REQUIRE(h, B >= 1 && B <= 8, "predict_mean_grad_multi: B must be in [1, 8]");
  W128 wt{}, sc{};
  for (int b = 0; b < B; ++b)
    for (int d = 0; d < D; ++d) {
      const double l = ls[b * D + d];
      GPK_REQUIRE(h, l > 0.0, "predict_mean_grad_multi: length-scales must be positive");
      wt.v[b * 16 + d] = 1.0 / (l * l);
      sc.v[b * 16 + d] = y_std[b] * sf2[b] / (l * l);
    }
  // model groups of BS <= 4: the fewest groups, evenly filled (B = 6: two groups of 3)
  const int ng = (B + 3) / 4, bs = (B + ng - 1) / ng, d4 = (D + 3) / 4;
  for (int64_t m0 = 0; m0 < M; m0 += MG_PANEL) {
    const int64_t mc = M - m0 < MG_PANEL ? M - m0 : MG_PANEL;
    const int64_t nqb = (mc + 255) / 256;
    // the chunking of gpk_predict_mean_grad
    const int64_t gran = (mc <= 512 && N <= 16384) ? 32 : JG_TJ;
    int64_t S = (2048 + nqb * ng - 1) / (nqb * ng);
    const int64_t maxS = (N + gran - 1) / gran;
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    if (S > 65535) S = 65535;
    int64_t chunk = (N + S - 1) / S;
    chunk = (chunk + gran - 1) / gran * gran;
    S = (N + chunk - 1) / chunk;
    if (h->gram_log)
      fprintf(stderr, "GPKDERIV mean_grad_multi %lld %d %d %lld d4%d bs%d ng%d nrb1 nqb%lld gran%lld s%lld chunk%lld\n", (long long)N, D,
              B, (long long)mc, d4, bs, ng, (long long)nqb, (long long)gran, (long long)S, (long long)chunk);
    void* partial = nullptr;
    GPK_TRY(gpk_scratch(h, (size_t)S * mc * B * D * sizeof(double), &partial));
    hipLaunchKernelGGL(mgm_pick(d4, bs), dim3((unsigned)nqb, (unsigned)S, (unsigned)ng), dim3(256), 0, h->stream, X, alpha,
                       (long long)N, D, B, wt, Xq + m0 * D, (long long)mc, (long long)chunk, (double*)partial);
    GPK_LAUNCH_CHECK(h);
    const int64_t tot = mc * B * D;
    hipLaunchKernelGGL(mean_grad_reduce_multi_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)partial, (int)S, (long long)mc, D, B, sc, dmean + m0 * B * D);
    GPK_LAUNCH_CHECK(h);
  }
  return GPK_OK;
}

extern "C" int gpk_predict_var_grad_inv(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2,
                                        const double* W, int64_t Np, int64_t ldw, const double* Xq, int64_t M, double kss,
                                        double floor_, double* work, double* var, double* dvar) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && W && Xq && work && dvar, "predict_var_grad_inv: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1 && Np == gpk_padded(N) && ldw >= Np, "predict_var_grad_inv: Np must equal gpk_padded(N), ldw >= Np");
  GPK_REQUIRE(h, h->batch == 1, "predict_var_grad_inv: not available in batched mode");
  Ls16 l;
  GPK_TRY(fill_ls16(h, ls, D, l));
  const int64_t Mp = gpk_padded(M);
  GPK_REQUIRE(h, Mp < (1ll << 31) && Np < (1ll << 31), "predict_var_grad_inv: size too large");
  double* Kt = work;                        // K*  (Np x Mp, training-major; zero in the padding)
  double* V = Kt + (size_t)Np * Mp;         // V = W K*
  double* Cm = V + (size_t)Np * Mp;         // C = W^T V = K^-1 K*
  GPK_TRY(gpk_cross_gram_t(h, GPK_F64, X, N, Xq, M, D, ls, sf2, Kt, Mp));
  // V = W K* with the plain store; W lower: tile row tm needs k < (tm + 1) * 128
  GemmArgs g1 = gemm_args(W, ldw, 0, Kt, Mp, 1, V, Mp, (int)Np, (int)Mp, (int)Np, 1.0, 0.0);
  g1.ke0 = GPK_TILE;
  g1.ke_row = GPK_TILE;
  g1.k_super = 1;            // W is zero right of the diagonal for GPK_ZERO_BAND_TILES - 1 tiles (gpk_trtri)
  g1.heavy_first = 1;
  GPK_TRY(gpk_gemm(h, GPK_F64, g1));
  // C = W^T V: C[i][m] = sum_{k >= i} W[k][i] V[k][m] - tile row tm needs k >= tm * 128 (the operand form of gpk_wtw)
  GemmArgs g2 = gemm_args(W, ldw, 1, V, Mp, 1, Cm, Mp, (int)Np, (int)Mp, (int)Np, 1.0, 0.0);
  g2.kb_row = GPK_TILE;
  g2.k_super = 1;
  gpk_time_begin(h, GPK_TIMED_JAC);
  const int rc_gemm = gpk_gemm(h, GPK_F64, g2);
  gpk_time_end(h);
  GPK_TRY(rc_gemm);
  // one streaming pass over the three panels, the training rows cut into chunks for ~2048 workgroups
  const int64_t ncb = (M + VG_COLS - 1) / VG_COLS;
  int64_t S = (2048 + ncb - 1) / ncb;
  const int64_t maxS = (N + VG_TJ - 1) / VG_TJ;
  if (S > maxS) S = maxS;
  if (S < 1) S = 1;
  int64_t chunk = (N + S - 1) / S;
  chunk = (chunk + VG_TJ - 1) / VG_TJ * VG_TJ;
  S = (N + chunk - 1) / chunk;
  if (h->gram_log)
    fprintf(stderr, "GPKDERIV var_grad %lld %d 1 %lld d4%d ps1 ng1 nrb1 ncb%lld gran%d s%lld chunk%lld\n", (long long)N, D, (long long)M,
            (D + 3) / 4, (long long)ncb, VG_TJ, (long long)S, (long long)chunk);
  void* pg = nullptr;
  GPK_TRY(gpk_scratch(h, (size_t)S * M * (D + 1) * sizeof(double), &pg));
  hipLaunchKernelGGL(vg_pick((D + 3) / 4), dim3((unsigned)ncb, (unsigned)S), dim3(VG_COLS), 0, h->stream, X, (long long)N, D, l,
                     Xq, (long long)M, (const double*)Kt, (const double*)Cm, (const double*)V, (long long)Mp, (long long)chunk,
                     (double*)pg);
  GPK_LAUNCH_CHECK(h);
  const int64_t tot = M * (D + 1);
  hipLaunchKernelGGL(var_grad_finalize_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, (const double*)pg,
                     (int)S, (long long)M, D, l, kss, floor_, var, dvar);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}
