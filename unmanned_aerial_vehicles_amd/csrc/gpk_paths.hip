// K10: posterior function draws by pathwise conditioning (gfx950, fp64).
//
// A path set for S paths and P outputs is ONE coefficient matrix Coef ((N + F) x C, C = S P, column s P + p, row-major, no row
// padding): rows [0, N) weight k(x, x_j), rows [N, N + F) weight cos(omega_f . x + phase_f) - the scale sqrt(2 sf2 / F) of the
// random Fourier features is folded into those rows.  Path s at a point x, output p:
//     out = y_mean[p] + y_std[p] sum_j b_j(x) Coef[j][s P + p]
//
//   rff_kernel            Phi[n][f] = scale cos(omega_f . x_n + phase_f) in the padded shape of the tile GEMM (zeros in the padding)
//   paths_pack_kernel     the operands of a set-up's products in the padded shape: W_rand and one more row block, copied (the
//                         sparse model's Xi) or as R = Yn (x) 1_S - Eps (the exact model)
//   paths_unpack_kernel   Coef from V (the exact model: V = K^-1 R; the sparse model: alpha_u + V) and scale W_rand
//   paths_partial_kernel  the hot path: grid (blocks of 64 paths) x (row chunks).  A workgroup is four waves; lane l of a wave owns
//                         path 64 block + l while the basis value b_j(xq_s) is formed - once per (s, j), D fused multiply-adds and one
//                         exp or cos - and leaves it in the wave's own LDS slots; then lane l owns COLUMNS l, l + 64, ... of the
//                         block's 64 P columns, so every load of a coefficient row is one contiguous run of 64 doubles per wave and
//                         the row is read exactly once.  The four waves take the chunk's rows four at a time (16 per round), their
//                         sums meet in LDS in wave order, and the chunk's share goes to partial[chunk][column].
//   paths_combine_kernel  the shares added in chunk order (no atomics: the same bits every call), un-normalised; in a rollout
//                         also the advance x <- x + lin [x, u] + out, written as the next stage of the trajectory, which is where
//                         the next stage's launch reads its queries.
//   paths_partial_multi_kernel / paths_combine_multi_kernel / paths_advance_multi_kernel
//                         the same two launches for the per-axis batch: B single-output models on shared inputs, each with its own
//                         kernel, Coef model-major (see there); with OWNZ every model has its own basis points (the sparse batch)
//   paths_partial_grad_kernel / paths_combine_grad_kernel / paths_combine_multi_grad_kernel
//                         the gradient forms (the *_grad entries): value and input Jacobian of every path in the same two
//                         launches, one first launch for the single model, the batch and the batch with own basis points (see there)
// Host side: paths_setup is the frame of both set-ups (gpk_paths_prepare; gpk_paths_prepare_two for a sparse model: N := m,
// X := Z, rows [0, m) hold v = alpha_u + WS^T xi - Wuu^T (Wuu Phi_Z w) from the two inverse factors of the assembled model), and
// paths_rollout_run drives every rollout: one device block, two uploads, H stages of two launches, one download.
// The chunk count depends on (N + F, S) only.  The launch is bound by streaming Coef: (N + F) S P 8 bytes per stage.
#include "gpk_internal.h"
#include "gpk_math.h"

namespace {

constexpr int PB = 64;        // paths per workgroup: one per lane
constexpr int PW = 4;         // waves per workgroup
constexpr int PR = 4;         // rows per wave and round
constexpr int PATHS_MAX_S = 4096, PATHS_MAX_F = 16384, PATHS_MAX_H = 256;
constexpr int PATHS_TARGET_WGS = 512;   // two workgroups per CU
constexpr int PATHS_MAX_CHUNKS = 512;

struct PathsK {
  double inv_ls[16];
  double ymean[16], ystd[16];
};

__global__ __launch_bounds__(256) void rff_kernel(const double* __restrict__ X, long long N, int D,
                                                  const double* __restrict__ Omega, const double* __restrict__ phase,
                                                  long long F, double scale, double* __restrict__ Phi, long long Fp,
                                                  long long ldp) {
  const long long n = blockIdx.y;
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= Fp) return;
  double v = 0.0;
  if (n < N && f < F) {
    double t = phase[f];
    for (int d = 0; d < D; ++d) t = __builtin_fma(Omega[f * D + d], X[n * D + d], t);
    v = scale * cos(t);
  }
  Phi[n * ldp + f] = v;
}

// Ap (np x Cp) = A[i][c], or with Yn: Yn[i][c % P] - A[i][c]; Wr (Fp x Cp) = W_rand[f][c]; zeros in the padding of both
__global__ __launch_bounds__(256) void paths_pack_kernel(const double* __restrict__ Yn, const double* __restrict__ A,
                                                         const double* __restrict__ Wrand, long long n, long long np, long long F,
                                                         long long C, long long Cp, int P, double* __restrict__ Ap,
                                                         double* __restrict__ Wr) {
  const long long row = blockIdx.y;      // [0, np): Ap; [np, np + Fp): Wr
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= Cp) return;
  if (row < np) {
    double v = 0.0;
    if (row < n && c < C) v = Yn ? Yn[row * P + c % P] - A[row * C + c] : A[row * C + c];
    Ap[row * Cp + c] = v;
  } else {
    const long long f = row - np;
    Wr[f * Cp + c] = (f < F && c < C) ? Wrand[f * C + c] : 0.0;
  }
}

// Coef rows [0, n): V[i][c], or with alpha: alpha[i][c % P] + V[i][c]; rows [n, n + F): scale W_rand
__global__ __launch_bounds__(256) void paths_unpack_kernel(const double* __restrict__ V, const double* __restrict__ alpha,
                                                           const double* __restrict__ Wrand, long long n, long long C,
                                                           long long Cp, int P, double scale, double* __restrict__ Coef,
                                                           long long ldc) {
  const long long row = blockIdx.y;      // [0, n + F)
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double v;
  if (row >= n) v = scale * Wrand[(row - n) * C + c];
  else v = alpha ? alpha[row * P + c % P] + V[row * Cp + c] : V[row * Cp + c];
  Coef[row * ldc + c] = v;
}

// The query of path s: its first dx coordinates from xs (S x dx), the others - shared by all paths - from u (D - dx).
template <int P>
__global__ __launch_bounds__(256) void paths_partial_kernel(const double* __restrict__ X, int N, int D, double sf2,
                                                            const double* __restrict__ Omega, const double* __restrict__ phase,
                                                            int F, const double* __restrict__ Coef, long long ldc, int S,
                                                            PathsK k, const double* __restrict__ xs, int dx,
                                                            const double* __restrict__ u, int rows_per_chunk,
                                                            double* __restrict__ partial) {
  __shared__ double bs[PW][PR][PB];      // basis values: slot [w] is wave w's own
  __shared__ double red[PW][P][PB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = S * P, rows = N + F;
  const int s = min((int)blockIdx.x * PB + lane, S - 1);      // (a lane past the last path repeats it: its columns are never stored)
  const long long c0 = (long long)blockIdx.x * PB * P;
  const int r0 = (int)blockIdx.y * rows_per_chunk, r1 = min(r0 + rows_per_chunk, rows);
  double q[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) q[d] = d < dx ? xs[(long long)s * dx + d] : (d < D ? u[d - dx] : 0.0);
  double acc[P];
#pragma unroll
  for (int i = 0; i < P; ++i) acc[i] = 0.0;
  // every wave runs the same number of rounds; a row past the chunk contributes an exact zero
  for (int rb = r0; rb < r1; rb += PW * PR) {
#pragma unroll
    for (int r = 0; r < PR; ++r) {
      const int j = rb + r * PW + w;       // wave-uniform
      double b = 0.0;
      if (j < r1) {
        if (j < N) {
          const double* xj = X + (long long)j * D;
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < 16; ++d)
            if (d < D) {
              const double t = (q[d] - xj[d]) * k.inv_ls[d];
              d2 = __builtin_fma(t, t, d2);
            }
          b = sf2 * gpk_exp_neg(-0.5 * d2);
        } else {
          const double* om = Omega + (long long)(j - N) * D;
          double t = phase[j - N];
#pragma unroll
          for (int d = 0; d < 16; ++d)
            if (d < D) t = __builtin_fma(om[d], q[d], t);
          b = cos(t);
        }
      }
      bs[w][r][lane] = b;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();       // the slots are the wave's own: its LDS writes are in order before its reads
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double cv[PR][P];
#pragma unroll
    for (int r = 0; r < PR; ++r) {
      const int j = rb + r * PW + w;
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const long long c = c0 + lane + 64 * i;
        cv[r][i] = (j < r1 && c < C) ? Coef[(long long)j * ldc + c] : 0.0;
      }
    }
#pragma unroll
    for (int r = 0; r < PR; ++r)
#pragma unroll
      for (int i = 0; i < P; ++i) acc[i] = __builtin_fma(bs[w][r][(lane + 64 * i) / P], cv[r][i], acc[i]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();       // ... and its reads before the next round's writes
  }
#pragma unroll
  for (int i = 0; i < P; ++i) red[w][i][lane] = acc[i];
  __syncthreads();
  for (int e = tid; e < P * PB; e += 256) {
    const int i = e >> 6, l = e & 63;
    const long long c = c0 + l + 64 * i;
    if (c < C) {
      double t = red[0][i][l];
#pragma unroll
      for (int ww = 1; ww < PW; ++ww) t += red[ww][i][l];
      partial[(long long)blockIdx.y * C + c] = t;
    }
  }
}

// out[c] = y_mean[p] + y_std[p] sum over the chunks, in chunk order.  With x_next: out is not stored; column c = s P + p of the
// next stage is x[c] + lin[p] . [x_s, u] + that value (lin: P x D, row-major).
__global__ __launch_bounds__(256) void paths_combine_kernel(const double* __restrict__ partial, int chunks, int S, int P, int D,
                                                            PathsK k, double* __restrict__ out, const double* __restrict__ x,
                                                            const double* __restrict__ u, const double* __restrict__ lin,
                                                            double* __restrict__ x_next) {
  const int C = S * P;
  const int c = (int)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double t = 0.0;
#pragma unroll 8
  for (int ch = 0; ch < chunks; ++ch) t += partial[(long long)ch * C + c];
  const int p = c % P, s = c / P;
  const double v = __builtin_fma(k.ystd[p], t, k.ymean[p]);
  if (!x_next) {
    out[c] = v;
    return;
  }
  double a = 0.0;
  for (int d = 0; d < P; ++d) a = __builtin_fma(lin[p * D + d], x[(long long)s * P + d], a);
  for (int d = P; d < D; ++d) a = __builtin_fma(lin[p * D + d], u[d - P], a);
  x_next[c] = (x[c] + a) + v;
}

// rows per chunk and chunk count: a function of (N + F, S) only
void paths_chunks(long long rows, int S, int* rows_per_chunk, int* chunks) {
  const int pblocks = (S + PB - 1) / PB;
  long long want = (PATHS_TARGET_WGS + pblocks - 1) / pblocks;
  if (want > PATHS_MAX_CHUNKS) want = PATHS_MAX_CHUNKS;
  const int round = PW * PR;
  long long rpc = (rows + want - 1) / want;
  rpc = (rpc + round - 1) / round * round;
  *rows_per_chunk = (int)rpc;
  *chunks = (int)((rows + rpc - 1) / rpc);
}

int paths_fill_k(gpk_handle h, int D, int P, const double* ls, const double* y_mean, const double* y_std, PathsK& k) {
  GPK_REQUIRE(h, ls && y_mean && y_std, "paths: null length-scale or normalisation array");
  for (int d = 0; d < 16; ++d) k.inv_ls[d] = 0.0;
  for (int d = 0; d < D; ++d) {
    GPK_REQUIRE(h, ls[d] > 0.0, "length-scales must be positive");
    k.inv_ls[d] = 1.0 / ls[d];
  }
  for (int p = 0; p < 16; ++p) {
    k.ymean[p] = p < P ? y_mean[p] : 0.0;
    k.ystd[p] = p < P ? y_std[p] : 1.0;
  }
  return GPK_OK;
}

constexpr int PATHS_MAX_B = 8;      // models of a per-axis batch
constexpr int PATHS_GRAD_PG = 3;    // outputs of a single model per workgroup of the gradient kernel

// the shape limits every entry of the family shares; `outputs`: the entry's own count (P or B), refused with `outputs_msg`
int paths_check_shape(gpk_handle h, int64_t N, int D, int64_t F, int S, bool outputs_ok, const char* outputs_msg) {
  GPK_REQUIRE(h, h->batch == 1, "paths: not available in batched mode");
  GPK_REQUIRE(h, N >= 1 && N < (1ll << 30), "paths: N must be at least 1");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT, "paths: D must be in [1, 16]");
  GPK_REQUIRE(h, outputs_ok, outputs_msg);
  GPK_REQUIRE(h, S >= 1 && S <= PATHS_MAX_S, "paths: S must be in [1, 4096]");
  GPK_REQUIRE(h, F >= 1 && F <= PATHS_MAX_F, "paths: F must be in [1, 16384]");
  return GPK_OK;
}

int paths_check_single(gpk_handle h, int64_t N, int D, int64_t F, int S, int P, int64_t ldc) {
  GPK_TRY(paths_check_shape(h, N, D, F, S, P >= 1 && P <= GPK_MAX_P, "paths: P must be in [1, 16]"));
  GPK_REQUIRE(h, ldc >= (int64_t)S * P, "paths: ldc must be >= S * P");
  return GPK_OK;
}

int paths_check_multi(gpk_handle h, int64_t N, int D, int B, int64_t F, int S, int64_t ldc, int64_t mstride) {
  GPK_TRY(paths_check_shape(h, N, D, F, S, B >= 1 && B <= PATHS_MAX_B, "paths: B must be in [1, 8]"));
  GPK_REQUIRE(h, mstride >= S, "paths: mstride must be >= S");
  GPK_REQUIRE(h, ldc >= (int64_t)B * mstride, "paths: ldc must be >= B * mstride");
  return GPK_OK;
}

struct PathsModel {
  const double* X;
  int N, D;
  double sf2;
  const double* Omega;
  const double* phase;
  int F;
  const double* Coef;
  long long ldc;
  int S, P;
  PathsK k;
};

// one stage: the shares of every chunk, then their sum (out) or the advance (x_next)
int paths_stage(gpk_handle h, const PathsModel& m, const double* xs, int dx, const double* u, int rpc, int chunks, double* partial,
                double* out, const double* lin, double* x_next) {
  const dim3 grid((unsigned)((m.S + PB - 1) / PB), (unsigned)chunks);
#define GPK_PATHS(PP)                                                                                                          \
  case PP:                                                                                                                     \
    hipLaunchKernelGGL(paths_partial_kernel<PP>, grid, dim3(256), 0, h->stream, m.X, m.N, m.D, m.sf2, m.Omega, m.phase, m.F,   \
                       m.Coef, m.ldc, m.S, m.k, xs, dx, u, rpc, partial);                                                      \
    break
  switch (m.P) {
    GPK_PATHS(1); GPK_PATHS(2); GPK_PATHS(3); GPK_PATHS(4); GPK_PATHS(5); GPK_PATHS(6); GPK_PATHS(7); GPK_PATHS(8);
    GPK_PATHS(9); GPK_PATHS(10); GPK_PATHS(11); GPK_PATHS(12); GPK_PATHS(13); GPK_PATHS(14); GPK_PATHS(15); GPK_PATHS(16);
  }
#undef GPK_PATHS
  GPK_LAUNCH_CHECK(h);
  const int C = m.S * m.P;
  hipLaunchKernelGGL(paths_combine_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, h->stream, (const double*)partial,
                     chunks, m.S, m.P, m.D, m.k, out, xs, u, lin, x_next);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

// ---- the per-axis batch: B single-output models on shared inputs, each with its own kernel -------------------------------------
// Coef is model-major: model b, path s is column b mstride + s, so lane l of a wave owns path 64 block + l for the basis value AND
// for the product - no LDS between the two - and a wave's load of a coefficient row is B contiguous runs of 64 doubles.  The
// difference q_d - x_jd and the load of x_j are formed once per (s, j) for all B models; everything after that is the
// single-model kernel's arithmetic in the single-model kernel's order (chunking, rows rb + r PW + w with r ascending, waves in
// wave order, chunks in chunk order), so column b of the result has the bits of gpk_paths_step on model b's own path set.
struct PathsMultiK {
  double inv_ls[PATHS_MAX_B][16];
  double sf2[PATHS_MAX_B], shift[PATHS_MAX_B], scale[PATHS_MAX_B];
  double in_shift[16], in_scale[16];      // rollout: the shared input scaler, z = (q - in_shift) / in_scale
  int scaled;                             // 0: the queries are taken as they are
  int model_of[16];                       // rollout: the model whose output state coordinate i receives, -1: none
};

// partial[(chunk B + b) S + s]: the share of the chunk's rows in model b's sum for path s
// OWNZ: every model has its own basis points (the sparse models' inducing inputs): X is (B x N x D), model b's x_j at
// X + (b N + j) D - still a wave-uniform address - and the difference is formed per model; the expression forms
// (q_d - x_jd) inv_ls, fma(t, t, d2), sf2 exp(-d2 / 2) and every order are those of the shared form and of the single-model kernel.
template <int B, bool OWNZ>
__global__ __launch_bounds__(256) void paths_partial_multi_kernel(const double* __restrict__ X, int N, int D,
                                                                  const double* __restrict__ Omega,
                                                                  const double* __restrict__ phase, int F,
                                                                  const double* __restrict__ Coef, long long ldc,
                                                                  long long mstride, int S, PathsMultiK k,
                                                                  const double* __restrict__ xs, int dx,
                                                                  const double* __restrict__ u, int rows_per_chunk,
                                                                  double* __restrict__ partial) {
  __shared__ double red[PW][B][PB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rows = N + F;
  const int sp = (int)blockIdx.x * PB + lane;
  const bool live = sp < S;
  const int s = min(sp, S - 1);      // (a lane past the last path repeats it: its coefficients are zeros, its sums are never stored)
  const int r0 = (int)blockIdx.y * rows_per_chunk, r1 = min(r0 + rows_per_chunk, rows);
  double q[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) q[d] = d < dx ? xs[(long long)s * dx + d] : (d < D ? u[d - dx] : 0.0);
  if (k.scaled) {
#pragma unroll
    for (int d = 0; d < 16; ++d)
      if (d < D) q[d] = (q[d] - k.in_shift[d]) / k.in_scale[d];
  }
  double acc[B];
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b] = 0.0;
  const double* cs = Coef + s;
  // Wave w takes the chunk's rows r0 + w, r0 + w + PW, ... in ascending order - the order of the single-model kernel, whose rounds
  // of PR rows only keep more loads in flight.  One row at a time here: measured at B = 6, S = 500, rounds of 2 or 4 rows are 5 %
  // slower (the launch is bound by the B exp / cos per (s, j), and fewer registers give three waves per SIMD instead of two).
  for (int j = r0 + w; j < r1; j += PW) {      // j is wave-uniform
    double cv[B];
#pragma unroll
    for (int b = 0; b < B; ++b) cv[b] = live ? cs[(long long)j * ldc + b * mstride] : 0.0;
    double bv[B];
    if (j < N) {
      if constexpr (OWNZ) {
#pragma unroll
        for (int b = 0; b < B; ++b) {
          const double* xj = X + ((long long)b * N + j) * D;
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < 16; ++d)
            if (d < D) {
              const double t = (q[d] - xj[d]) * k.inv_ls[b][d];
              d2 = __builtin_fma(t, t, d2);
            }
          bv[b] = k.sf2[b] * gpk_exp_neg(-0.5 * d2);
        }
      } else {
        const double* xj = X + (long long)j * D;
        double df[16];
#pragma unroll
        for (int d = 0; d < 16; ++d) df[d] = d < D ? q[d] - xj[d] : 0.0;
#pragma unroll
        for (int b = 0; b < B; ++b) {
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < 16; ++d)
            if (d < D) {
              const double t = df[d] * k.inv_ls[b][d];
              d2 = __builtin_fma(t, t, d2);
            }
          bv[b] = k.sf2[b] * gpk_exp_neg(-0.5 * d2);
        }
      }
    } else {
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const long long f = (long long)b * F + (j - N);
        const double* om = Omega + f * D;
        double t = phase[f];
#pragma unroll
        for (int d = 0; d < 16; ++d)
          if (d < D) t = __builtin_fma(om[d], q[d], t);
        bv[b] = cos(t);
      }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b] = __builtin_fma(bv[b], cv[b], acc[b]);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) red[w][b][lane] = acc[b];
  __syncthreads();
  for (int e = tid; e < B * PB; e += 256) {
    const int b = e >> 6, l = e & 63;
    const int sl = (int)blockIdx.x * PB + l;
    if (sl < S) {
      double t = red[0][b][l];
#pragma unroll
      for (int ww = 1; ww < PW; ++ww) t += red[ww][b][l];
      partial[((long long)blockIdx.y * B + b) * S + sl] = t;
    }
  }
}

// grid (blocks of 256 paths) x B: out[s][b] = shift[b] + scale[b] sum over the chunks, in chunk order
__global__ __launch_bounds__(256) void paths_combine_multi_kernel(const double* __restrict__ partial, int chunks, int S, int B,
                                                                  PathsMultiK k, double* __restrict__ out) {
  const int b = blockIdx.y;
  const int s = (int)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  double t = 0.0;
#pragma unroll 8
  for (int ch = 0; ch < chunks; ++ch) t += partial[((long long)ch * B + b) * S + s];
  out[(long long)s * B + b] = __builtin_fma(k.scale[b], t, k.shift[b]);
}

// grid (blocks of 256 paths) x nx, the advance of a rollout: coordinate i of the next stage is x_i + lin[i] . [x_s, u] plus, where
// a model feeds that coordinate, its value; x and u in raw units (lin: nx x D, row-major)
__global__ __launch_bounds__(256) void paths_advance_multi_kernel(const double* __restrict__ partial, int chunks, int S, int B,
                                                                  int nx, int D, PathsMultiK k, const double* __restrict__ x,
                                                                  const double* __restrict__ u, const double* __restrict__ lin,
                                                                  double* __restrict__ x_next) {
  const int i = blockIdx.y;
  const int s = (int)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const double* xr = x + (long long)s * nx;
  double a = 0.0;
  for (int d = 0; d < nx; ++d) a = __builtin_fma(lin[i * D + d], xr[d], a);
  for (int d = nx; d < D; ++d) a = __builtin_fma(lin[i * D + d], u[d - nx], a);
  double v = xr[i] + a;
  const int b = k.model_of[i];
  if (b >= 0) {
    double t = 0.0;
#pragma unroll 8
    for (int ch = 0; ch < chunks; ++ch) t += partial[((long long)ch * B + b) * S + s];
    v += __builtin_fma(k.scale[b], t, k.shift[b]);
  }
  x_next[(long long)s * nx + i] = v;
}

struct PathsMultiModel {
  const double* X;      // own_z: (B x N x D), every model's own basis points
  bool own_z;
  int N, D, B;
  const double* Omega;
  const double* phase;
  int F;
  const double* Coef;
  long long ldc, mstride;
  int S;
  PathsMultiK k;
};

int paths_fill_multi(gpk_handle h, int D, int B, const double* ls, const double* sf2, const double* shift, const double* scale,
                     PathsMultiK& k) {
  GPK_REQUIRE(h, ls && sf2 && shift && scale, "paths: null length-scale, sf2, shift or scale array");
  for (int b = 0; b < PATHS_MAX_B; ++b) {
    for (int d = 0; d < 16; ++d) k.inv_ls[b][d] = 0.0;
    k.sf2[b] = 0.0;
    k.shift[b] = 0.0;
    k.scale[b] = 1.0;
  }
  for (int b = 0; b < B; ++b) {
    for (int d = 0; d < D; ++d) {
      GPK_REQUIRE(h, ls[b * D + d] > 0.0, "length-scales must be positive");
      k.inv_ls[b][d] = 1.0 / ls[b * D + d];
    }
    k.sf2[b] = sf2[b];
    k.shift[b] = shift[b];
    k.scale[b] = scale[b];
  }
  for (int d = 0; d < 16; ++d) {
    k.in_shift[d] = 0.0;
    k.in_scale[d] = 1.0;
    k.model_of[d] = -1;
  }
  k.scaled = 0;
  return GPK_OK;
}

// the first launch of a stage: the shares of every chunk
int paths_partial_multi(gpk_handle h, const PathsMultiModel& m, const double* xs, int dx, const double* u, int rpc, int chunks,
                        double* partial) {
  const dim3 grid((unsigned)((m.S + PB - 1) / PB), (unsigned)chunks);
#define GPK_PATHS_MULTI(BB)                                                                                                    \
  case BB:                                                                                                                     \
    if (m.own_z)                                                                                                               \
      hipLaunchKernelGGL((paths_partial_multi_kernel<BB, true>), grid, dim3(256), 0, h->stream, m.X, m.N, m.D, m.Omega,        \
                         m.phase, m.F, m.Coef, m.ldc, m.mstride, m.S, m.k, xs, dx, u, rpc, partial);                           \
    else                                                                                                                       \
      hipLaunchKernelGGL((paths_partial_multi_kernel<BB, false>), grid, dim3(256), 0, h->stream, m.X, m.N, m.D, m.Omega,       \
                         m.phase, m.F, m.Coef, m.ldc, m.mstride, m.S, m.k, xs, dx, u, rpc, partial);                           \
    break
  switch (m.B) {
    GPK_PATHS_MULTI(1); GPK_PATHS_MULTI(2); GPK_PATHS_MULTI(3); GPK_PATHS_MULTI(4);
    GPK_PATHS_MULTI(5); GPK_PATHS_MULTI(6); GPK_PATHS_MULTI(7); GPK_PATHS_MULTI(8);
  }
#undef GPK_PATHS_MULTI
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

// ---- the gradient forms: value and input Jacobian of every path in the same two launches ---------------------------------------
// d/dx_d of sum_j b_j(x) c_j:  RBF rows  -inv_ls_d sum_j e_j t_jd  (e_j = b_j c_j, t_jd = (x_d - x_jd) inv_ls_d, the t the value
// forms), cosine rows  -sum_f e'_f omega_fd  (e'_f = sin(t_f) c_f).  ONE kernel serves both layouts: the output (p of a single
// model, b of a batch) is the grid's third dimension, lane l owns path 64 block + l for the basis value, the product and the D
// derivative sums alike, and the layout is a pair of strides (coefficient column s cs + o co, share column s ps + o po).  A
// workgroup keeps PG (1 + D) sums per lane whatever P or B is (PG <= 3 outputs of a single model, which share the basis value and
// the t_d; one model of a batch).  Rows, waves and chunks go in the order of the value kernels and the
// value is formed by their expressions, so the value shares have the bits of paths_partial_kernel / paths_partial_multi_kernel.
// The two kinds of row need different factors afterwards, so their derivative shares are kept apart: area ch of gpart holds
// chunk ch's RBF rows if the chunk starts below N and its cosine rows otherwise; the cosine rows of the one chunk that
// holds row N and rows above it go to area `chunks`.
struct PathsGradK {
  double inv_ls[PATHS_MAX_B][16];
  double sf2[PATHS_MAX_B];
  double in_shift[16], in_scale[16];      // as PathsMultiK
  int scaled;
  int per_model;                          // 1: output o has its own kernel (row o of inv_ls, sf2), 0: row 0 serves all
};

struct PathsGradModel {
  const double* X;
  int N, D;
  long long xstride;      // doubles between the basis points of two outputs (0: shared)
  const double* Omega;
  const double* phase;
  int F;
  long long fstride;      // features between two outputs (0: shared)
  const double* Coef;
  long long ldc, cs, co;  // coefficient column of (path s, output o): s cs + o co
  int S, nout;
  long long ps, po;       // share column of (s, o): s ps + o po, below C = S nout
  PathsGradK k;
};

// the D sums of a workgroup's four waves, added in wave order, to area `area` of gpart ((areas x D x C), column col)
__device__ __forceinline__ void paths_grad_store(double (*red)[16][PB], const double (&G)[16], int D, int w, int lane, int tid,
                                                 int S, long long C, long long ps, long long pcol0, long long area,
                                                 double* __restrict__ gpart) {
#pragma unroll
  for (int d = 0; d < 16; ++d)
    if (d < D) red[w][d][lane] = G[d];
  __syncthreads();
  for (int e = tid; e < D * PB; e += 256) {
    const int d = e >> 6, l = e & 63;
    const int sl = (int)blockIdx.x * PB + l;
    if (sl < S) {
      double t = red[0][d][l];
#pragma unroll
      for (int ww = 1; ww < PW; ++ww) t += red[ww][d][l];
      gpart[(area * D + d) * C + pcol0 + sl * ps] = t;
    }
  }
  __syncthreads();
}

// PG: the outputs a workgroup serves, o0 = PG blockIdx.z and the next ones (a single model's p share the basis value and the
// t_d; a batch's models share nothing: PG = 1).  Every output's sums are formed by the same expressions whatever PG is.
template <int PG>
__global__ __launch_bounds__(256) void paths_partial_grad_kernel(PathsGradModel m, const double* __restrict__ xs, int dx,
                                                                 const double* __restrict__ u, int rows_per_chunk, int chunks,
                                                                 double* __restrict__ partial, double* __restrict__ gpart) {
  __shared__ double red[PW][16][PB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = m.N, D = m.D, S = m.S, rows = N + m.F;
  const int o0 = (int)blockIdx.z * PG, mi = m.k.per_model ? o0 : 0;
  const int sp = (int)blockIdx.x * PB + lane;
  const bool live = sp < S;
  const int s = min(sp, S - 1);      // (a lane past the last path repeats it: its coefficients are zeros, its sums are never stored)
  const int r0 = (int)blockIdx.y * rows_per_chunk, r1 = min(r0 + rows_per_chunk, rows);
  const long long C = (long long)S * m.nout, pcol0 = o0 * m.po;
  double q[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) q[d] = d < dx ? xs[(long long)s * dx + d] : (d < D ? u[d - dx] : 0.0);
  if (m.k.scaled) {
#pragma unroll
    for (int d = 0; d < 16; ++d)
      if (d < D) q[d] = (q[d] - m.k.in_shift[d]) / m.k.in_scale[d];
  }
  const double* __restrict__ Xo = m.X + o0 * m.xstride;
  const double* __restrict__ Om = m.Omega + o0 * m.fstride * D;
  const double* __restrict__ ph = m.phase + o0 * m.fstride;
  const double* __restrict__ cp = m.Coef + s * m.cs + o0 * m.co;
  const double sf2 = m.k.sf2[mi];
  bool on[PG];      // (uniform) the group's last outputs may lie past nout: their coefficients are zeros, their sums are never stored
#pragma unroll
  for (int g = 0; g < PG; ++g) on[g] = o0 + g < m.nout;
  double acc[PG], G[PG][16];
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    acc[g] = 0.0;
#pragma unroll
    for (int d = 0; d < 16; ++d) G[g][d] = 0.0;
  }
  // wave w takes the chunk's rows r0 + w, r0 + w + PW, ... in ascending order (j is wave-uniform): first those below N ...
  const int nA = min(r1, N);
  int j = r0 + w;
  for (; j < nA; j += PW) {
    double cv[PG];
#pragma unroll
    for (int g = 0; g < PG; ++g) cv[g] = (live && on[g]) ? cp[(long long)j * m.ldc + g * m.co] : 0.0;
    const double* xj = Xo + (long long)j * D;
    double t[16], d2 = 0.0;
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      t[d] = 0.0;
      if (d < D) {
        t[d] = (q[d] - xj[d]) * m.k.inv_ls[mi][d];
        d2 = __builtin_fma(t[d], t[d], d2);
      }
    }
    const double b = sf2 * gpk_exp_neg(-0.5 * d2);
#pragma unroll
    for (int g = 0; g < PG; ++g) {
      acc[g] = __builtin_fma(b, cv[g], acc[g]);
      const double e = b * cv[g];
#pragma unroll
      for (int d = 0; d < 16; ++d)
        if (d < D) G[g][d] = __builtin_fma(e, t[d], G[g][d]);
    }
  }
  if (r0 < N) {      // (uniform over the workgroup)
#pragma unroll
    for (int g = 0; g < PG; ++g) {
      if (on[g]) paths_grad_store(red, G[g], D, w, lane, tid, S, C, m.ps, pcol0 + g * m.po, blockIdx.y, gpart);
#pragma unroll
      for (int d = 0; d < 16; ++d) G[g][d] = 0.0;
    }
  }
  // ... then the cosine rows
  for (; j < r1; j += PW) {
    double cv[PG];
#pragma unroll
    for (int g = 0; g < PG; ++g) cv[g] = (live && on[g]) ? cp[(long long)j * m.ldc + g * m.co] : 0.0;
    const double* om = Om + (long long)(j - N) * D;
    double t = ph[j - N];
#pragma unroll
    for (int d = 0; d < 16; ++d)
      if (d < D) t = __builtin_fma(om[d], q[d], t);
    const double b = cos(t), sn = sin(t);
#pragma unroll
    for (int g = 0; g < PG; ++g) {
      acc[g] = __builtin_fma(b, cv[g], acc[g]);
      const double e = sn * cv[g];
#pragma unroll
      for (int d = 0; d < 16; ++d)
        if (d < D) G[g][d] = __builtin_fma(e, om[d], G[g][d]);
    }
  }
  if (r1 > N) {
#pragma unroll
    for (int g = 0; g < PG; ++g)
      if (on[g])
        paths_grad_store(red, G[g], D, w, lane, tid, S, C, m.ps, pcol0 + g * m.po, r0 < N ? chunks : (int)blockIdx.y, gpart);
  }
  // the value's shares, as the value kernels form them
#pragma unroll
  for (int g = 0; g < PG; ++g) red[w][g][lane] = acc[g];
  __syncthreads();
  for (int e = tid; e < PG * PB; e += 256) {
    const int g = e >> 6, l = e & 63;
    const int sl = (int)blockIdx.x * PB + l;
    if (sl < S && o0 + g < m.nout) {
      double t = red[0][g][l];
#pragma unroll
      for (int ww = 1; ww < PW; ++ww) t += red[ww][g][l];
      partial[(long long)blockIdx.y * C + pcol0 + g * m.po + sl * m.ps] = t;
    }
  }
}

// One entry of the Jacobian from the derivative shares, in chunk order: the RBF areas (chunks that start below N), then the
// cosine areas - area `chunks` first, the chunk that holds row N, if it also holds rows above it.
__device__ __forceinline__ double paths_jac_entry(const double* __restrict__ gpart, int chunks, int rows_per_chunk, int N, int D,
                                                  long long C, long long col, int d, double inv_ls, double scale) {
  const int nr = (N + rows_per_chunk - 1) / rows_per_chunk;      // chunks that start below N
  const double* g = gpart + (long long)d * C + col;
  const long long step = (long long)D * C;
  double tr = 0.0;
#pragma unroll 8
  for (int ch = 0; ch < nr; ++ch) tr += g[ch * step];
  double tc = 0.0;
  if (N % rows_per_chunk != 0) tc += g[chunks * step];
#pragma unroll 8
  for (int ch = nr; ch < chunks; ++ch) tc += g[ch * step];
  return scale * -__builtin_fma(inv_ls, tr, tc);
}

// grid (blocks of 256 columns) x (1 + D): row 0 is paths_combine_kernel, row 1 + d writes jac[c][d]
__global__ __launch_bounds__(256) void paths_combine_grad_kernel(const double* __restrict__ partial,
                                                                 const double* __restrict__ gpart, int chunks, int rows_per_chunk,
                                                                 int N, int S, int P, int D, PathsK k, double* __restrict__ out,
                                                                 const double* __restrict__ x, const double* __restrict__ u,
                                                                 const double* __restrict__ lin, double* __restrict__ x_next,
                                                                 double* __restrict__ jac) {
  const int C = S * P;
  const int c = (int)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int p = c % P, s = c / P;
  if (blockIdx.y > 0) {
    const int d = (int)blockIdx.y - 1;
    jac[(long long)c * D + d] = paths_jac_entry(gpart, chunks, rows_per_chunk, N, D, C, c, d, k.inv_ls[d], k.ystd[p]);
    return;
  }
  double t = 0.0;
#pragma unroll 8
  for (int ch = 0; ch < chunks; ++ch) t += partial[(long long)ch * C + c];
  const double v = __builtin_fma(k.ystd[p], t, k.ymean[p]);
  if (!x_next) {
    out[c] = v;
    return;
  }
  double a = 0.0;
  for (int d = 0; d < P; ++d) a = __builtin_fma(lin[p * D + d], x[(long long)s * P + d], a);
  for (int d = P; d < D; ++d) a = __builtin_fma(lin[p * D + d], u[d - P], a);
  x_next[c] = (x[c] + a) + v;
}

// grid (blocks of 256 paths) x (nv + B D): rows [0, nv) are paths_combine_multi_kernel (nv = B, x_next null) or
// paths_advance_multi_kernel (nv = nx); row nv + b D + d writes jac[s][b][d], in a rollout per unit of the RAW query
__global__ __launch_bounds__(256) void paths_combine_multi_grad_kernel(const double* __restrict__ partial,
                                                                       const double* __restrict__ gpart, int chunks,
                                                                       int rows_per_chunk, int N, int S, int B, int nv, int D,
                                                                       PathsMultiK k, double* __restrict__ out,
                                                                       const double* __restrict__ x, const double* __restrict__ u,
                                                                       const double* __restrict__ lin, double* __restrict__ x_next,
                                                                       double* __restrict__ jac) {
  const int s = (int)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  if ((int)blockIdx.y >= nv) {
    const int b = ((int)blockIdx.y - nv) / D, d = ((int)blockIdx.y - nv) % D;
    double v = paths_jac_entry(gpart, chunks, rows_per_chunk, N, D, (long long)B * S, (long long)b * S + s, d, k.inv_ls[b][d],
                               k.scale[b]);
    if (x_next) v /= k.in_scale[d];
    jac[((long long)s * B + b) * D + d] = v;
    return;
  }
  if (!x_next) {
    const int b = blockIdx.y;
    double t = 0.0;
#pragma unroll 8
    for (int ch = 0; ch < chunks; ++ch) t += partial[((long long)ch * B + b) * S + s];
    out[(long long)s * B + b] = __builtin_fma(k.scale[b], t, k.shift[b]);
    return;
  }
  const int i = blockIdx.y, nx = nv;
  const double* xr = x + (long long)s * nx;
  double a = 0.0;
  for (int d = 0; d < nx; ++d) a = __builtin_fma(lin[i * D + d], xr[d], a);
  for (int d = nx; d < D; ++d) a = __builtin_fma(lin[i * D + d], u[d - nx], a);
  double v = xr[i] + a;
  const int b = k.model_of[i];
  if (b >= 0) {
    double t = 0.0;
#pragma unroll 8
    for (int ch = 0; ch < chunks; ++ch) t += partial[((long long)ch * B + b) * S + s];
    v += __builtin_fma(k.scale[b], t, k.shift[b]);
  }
  x_next[(long long)s * nx + i] = v;
}

// the first launch of a gradient stage: value shares (chunks x C) and derivative shares ((chunks + 1) x D x C)
int paths_partial_grad(gpk_handle h, const PathsGradModel& g, const double* xs, int dx, const double* u, int rpc, int chunks,
                       double* partial, double* gpart) {
  // a single model's outputs in groups of PATHS_GRAD_PG (they share the basis value); a batch's models one by one
  const int pg = g.k.per_model ? 1 : (g.nout < PATHS_GRAD_PG ? g.nout : PATHS_GRAD_PG);
  const dim3 grid((unsigned)((g.S + PB - 1) / PB), (unsigned)chunks, (unsigned)((g.nout + pg - 1) / pg));
#define GPK_PATHS_GRAD(PGG)                                                                                                    \
  case PGG:                                                                                                                    \
    hipLaunchKernelGGL(paths_partial_grad_kernel<PGG>, grid, dim3(256), 0, h->stream, g, xs, dx, u, rpc, chunks, partial,      \
                       gpart);                                                                                                 \
    break
  switch (pg) {
    GPK_PATHS_GRAD(1); GPK_PATHS_GRAD(2); GPK_PATHS_GRAD(3);
  }
#undef GPK_PATHS_GRAD
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

PathsGradModel paths_grad_model(const PathsModel& m) {
  PathsGradModel g{m.X, m.N, m.D, 0, m.Omega, m.phase, m.F, 0, m.Coef, m.ldc, m.P, 1, m.S, m.P, m.P, 1, {}};
  for (int d = 0; d < 16; ++d) {
    g.k.inv_ls[0][d] = m.k.inv_ls[d];
    g.k.in_shift[d] = 0.0;
    g.k.in_scale[d] = 1.0;
  }
  g.k.sf2[0] = m.sf2;
  return g;
}

PathsGradModel paths_grad_model(const PathsMultiModel& m) {
  PathsGradModel g{m.X, m.N, m.D, m.own_z ? (long long)m.N * m.D : 0, m.Omega, m.phase, m.F, m.F, m.Coef, m.ldc, 1, m.mstride,
                   m.S, m.B, 1, m.S, {}};
  for (int b = 0; b < PATHS_MAX_B; ++b) {
    for (int d = 0; d < 16; ++d) g.k.inv_ls[b][d] = m.k.inv_ls[b][d];
    g.k.sf2[b] = m.k.sf2[b];
  }
  for (int d = 0; d < 16; ++d) {
    g.k.in_shift[d] = m.k.in_shift[d];
    g.k.in_scale[d] = m.k.in_scale[d];
  }
  g.k.scaled = m.k.scaled;
  g.k.per_model = 1;
  return g;
}

// doubles of a gradient stage's shares: the value's, then the derivatives'
size_t paths_grad_shares(int chunks, int D, size_t C) { return (size_t)chunks * C + (size_t)(chunks + 1) * D * C; }

// one gradient stage of a single model: as paths_stage, and jac (S x P x D)
int paths_stage_grad(gpk_handle h, const PathsModel& m, const PathsGradModel& g, const double* xs, int dx, const double* u, int rpc,
                     int chunks, double* partial, double* out, const double* lin, double* x_next, double* jac) {
  const int C = m.S * m.P;
  double* gpart = partial + (size_t)chunks * C;
  GPK_TRY(paths_partial_grad(h, g, xs, dx, u, rpc, chunks, partial, gpart));
  hipLaunchKernelGGL(paths_combine_grad_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)(1 + m.D)), dim3(256), 0, h->stream,
                     (const double*)partial, (const double*)gpart, chunks, rpc, m.N, m.S, m.P, m.D, m.k, out, xs, u, lin, x_next,
                     jac);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

// one gradient stage of a batch: nv = B and out (a step) or nv = nx, lin and x_next (a rollout's advance), and jac (S x B x D)
int paths_stage_multi_grad(gpk_handle h, const PathsMultiModel& m, const PathsGradModel& g, const double* xs, int dx,
                           const double* u, int rpc, int chunks, double* partial, int nv, double* out, const double* lin,
                           double* x_next, double* jac) {
  double* gpart = partial + (size_t)chunks * m.S * m.B;
  GPK_TRY(paths_partial_grad(h, g, xs, dx, u, rpc, chunks, partial, gpart));
  hipLaunchKernelGGL(paths_combine_multi_grad_kernel, dim3((unsigned)((m.S + 255) / 256), (unsigned)(nv + m.B * m.D)), dim3(256), 0,
                     h->stream, (const double*)partial, (const double*)gpart, chunks, rpc, m.N, m.S, m.B, nv, m.D, m.k, out, xs, u,
                     lin, x_next, jac);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

// One closed-loop horizon, every kind of path set: the refusals the rollouts share, then the device block - the trajectory
// ((H + 1) x S x w), then [stage 0 | U | lin] as they come from the host in one copy (stage 0 is the trajectory's first slot) and
// the chunks' shares (n_partial doubles) - two uploads, H stages, one download, one synchronisation.  w: the state width, at most
// D (the entry's own check); stage(xk, uk, partial, d_lin, x_next, jac_k) launches one stage; `name` heads the messages.
// A gradient rollout (jac, host, H x n_jac) adds the Jacobian area to the block - stage k writes its n_jac doubles at jac_k -
// and one more download before the same synchronisation; without it n_jac = 0 and jac_k is null.
template <class Stage>
int paths_rollout_run(gpk_handle h, const char* name, int w, int D, int S, const double* x0, int x0_rows, const double* U, int H,
                      const double* lin, double* traj, size_t n_partial, size_t n_jac, double* jac, Stage stage) {
  const std::string who = std::string(name) + ": ";
  GPK_REQUIRE(h, H >= 1 && H <= PATHS_MAX_H, who + "H must be in [1, 256]");
  GPK_REQUIRE(h, x0_rows == 1 || x0_rows == S, who + "x0 must have 1 or S rows");
  const int du = D - w;
  GPK_REQUIRE(h, du == 0 || U, who + "null controls");
  GPK_REQUIRE(h, gpk_finite(x0, (long long)x0_rows * w) && gpk_finite(lin, (long long)w * D) &&
                     (du == 0 || gpk_finite(U, (long long)H * du)),
              who + "x0, U and lin must not contain NaN or infinity");
  const size_t C = (size_t)S * w;
  const size_t n_traj = (size_t)(H + 1) * C, n_u = (size_t)H * du, n_lin = (size_t)w * D;
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, (n_traj + n_u + n_lin + n_partial + (size_t)H * n_jac) * sizeof(double), &ws));
  double* d_traj = (double*)ws;
  double* d_u = d_traj + n_traj;
  double* d_lin = d_u + n_u;
  double* partial = d_lin + n_lin;
  double* d_jac = n_jac ? partial + n_partial : nullptr;
  std::vector<double> host(C + n_u + n_lin);
  for (int s = 0; s < S; ++s) memcpy(host.data() + (size_t)s * w, x0 + (x0_rows == 1 ? 0 : (size_t)s * w), sizeof(double) * w);
  if (n_u) memcpy(host.data() + C, U, sizeof(double) * n_u);
  memcpy(host.data() + C + n_u, lin, sizeof(double) * n_lin);
  GPK_CHECK_HIP(h, hipMemcpyAsync(d_traj, host.data(), sizeof(double) * C, hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(d_u, host.data() + C, sizeof(double) * (n_u + n_lin), hipMemcpyHostToDevice, h->stream));
  for (int k = 0; k < H; ++k)
    GPK_TRY(stage(d_traj + (size_t)k * C, d_u + (size_t)k * du, partial, (const double*)d_lin, d_traj + (size_t)(k + 1) * C,
                  d_jac ? d_jac + (size_t)k * n_jac : nullptr));
  GPK_CHECK_HIP(h, hipMemcpyAsync(traj, d_traj, sizeof(double) * n_traj, hipMemcpyDeviceToHost, h->stream));
  if (d_jac) GPK_CHECK_HIP(h, hipMemcpyAsync(jac, d_jac, sizeof(double) * H * n_jac, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  return GPK_OK;
}

// dst (np x Cp) = sign W^T (W src) through a lower inverse factor W (np x np tiles, row stride ldw), as gpk_potrs_inv: T = W src
// (W lower: k < row-tile end), dst = sign W^T T (k >= row-tile start).  The identity in W's padding keeps zero rows of src zero.
int paths_inverse_product(gpk_handle h, const double* W, int64_t ldw, int64_t np, int64_t Cp, const double* src, double* T,
                          double* dst, double sign) {
  GemmArgs g1 = gemm_args(W, ldw, 0, src, Cp, 1, T, Cp, (int)np, (int)Cp, (int)np, 1.0, 0.0);
  g1.ke0 = GPK_TILE; g1.ke_row = GPK_TILE; g1.heavy_first = 1;
  GPK_TRY(gpk_gemm(h, GPK_F64, g1));
  GemmArgs g2 = gemm_args(W, ldw, 1, T, Cp, 1, dst, Cp, (int)np, (int)Cp, (int)np, sign, 0.0);
  g2.kb_row = GPK_TILE;
  return gpk_gemm(h, GPK_F64, g2);
}

// The frame of both set-ups, over n basis points X (np = gpk_padded(n) rows in every padded shape).  Work area: Phi (np x Fp),
// Wr (Fp x Cp), then `areas` matrices M[0], M[1], ... of np x Cp.  Phi = the features of X, Wr = W_rand and M[0] = A (or
// Yn (x) 1_S - A) are filled; products(Phi, Wr, M, Cp, Fp) runs the entry's own GEMMs and leaves V in M[v_area]; Coef rows
// [0, n) = V (or alpha + V), rows [n, n + F) = scale W_rand.
template <class Products>
int paths_setup(gpk_handle h, const char* too_tall, const double* X, int64_t n, int64_t np, int D, int P, double sf2,
                const double* Omega, const double* phase, int64_t F, const double* W_rand, const double* Yn, const double* A,
                const double* alpha, int S, double* Coef, int64_t ldc, int areas, int v_area, Products products) {
  const int64_t C = (int64_t)S * P, Cp = gpk_padded(C), Fp = gpk_padded(F);
  GPK_REQUIRE(h, np + Fp <= 65535, too_tall);
  const double scale = sqrt(2.0 * sf2 / (double)F);
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, (size_t)(np * Fp + Fp * Cp + areas * np * Cp) * sizeof(double), &ws));
  double* Phi = (double*)ws;
  double* Wr = Phi + np * Fp;
  double* M = Wr + Fp * Cp;
  GPK_TRY(gpk_rff_features(h, X, n, D, Omega, phase, F, scale, Phi, Fp));
  hipLaunchKernelGGL(paths_pack_kernel, dim3((unsigned)(Cp / 256 + (Cp % 256 != 0)), (unsigned)(np + Fp)), dim3(256), 0, h->stream,
                     Yn, A, W_rand, (long long)n, (long long)np, (long long)F, (long long)C, (long long)Cp, P, M, Wr);
  GPK_LAUNCH_CHECK(h);
  GPK_TRY(products(Phi, Wr, M, Cp, Fp));
  hipLaunchKernelGGL(paths_unpack_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)(n + F)), dim3(256), 0, h->stream,
                     (const double*)(M + v_area * np * Cp), alpha, W_rand, (long long)n, (long long)C, (long long)Cp, P, scale, Coef,
                     (long long)ldc);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

}  // namespace

extern "C" int gpk_rff_features(gpk_handle h, const double* X, int64_t N, int D, const double* Omega, const double* phase,
                                int64_t F, double scale, double* Phi, int64_t ldp) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Omega && phase && Phi, "rff_features: null pointer");
  GPK_REQUIRE(h, N >= 1 && N < (1ll << 30), "rff_features: N must be at least 1");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT, "rff_features: D must be in [1, 16]");
  GPK_REQUIRE(h, F >= 1 && F <= PATHS_MAX_F, "rff_features: F must be in [1, 16384]");
  const int64_t Np = gpk_padded(N), Fp = gpk_padded(F);
  GPK_REQUIRE(h, ldp >= Fp, "rff_features: ldp must be >= gpk_padded(F)");
  // (rows go in the grid's y dimension, 65535 at a time)
  for (int64_t n0 = 0; n0 < Np; n0 += 65535) {
    const int64_t nr = Np - n0 < 65535 ? Np - n0 : 65535;
    hipLaunchKernelGGL(rff_kernel, dim3((unsigned)(Fp / 256 + (Fp % 256 != 0)), (unsigned)nr), dim3(256), 0, h->stream,
                       X + n0 * D, (long long)(N - n0 > 0 ? N - n0 : 0), D, Omega, phase, (long long)F, scale, Phi + n0 * ldp,
                       (long long)Fp, (long long)ldp);
    GPK_LAUNCH_CHECK(h);
  }
  return GPK_OK;
}

extern "C" int gpk_paths_prepare(gpk_handle h, const double* X, int64_t N, int D, const double* Yn, int P, const double* W,
                                 int64_t Np, int64_t ldw, const double* Omega, const double* phase, int64_t F, double sf2,
                                 const double* W_rand, const double* Eps, int S, double* Coef, int64_t ldc) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Yn && W && Omega && phase && W_rand && Eps && Coef, "paths_prepare: null pointer");
  GPK_TRY(paths_check_single(h, N, D, F, S, P, ldc));
  GPK_REQUIRE(h, Np == gpk_padded(N) && ldw >= Np, "paths_prepare: Np must equal gpk_padded(N) and ldw >= Np");
  GPK_REQUIRE(h, sf2 > 0.0, "paths_prepare: sf2 must be positive");
  // areas: R = Yn (x) 1_S - Eps, T.  R <- R - Phi Wr, then V = K^-1 R = W^T (W R), in place
  return paths_setup(h, "paths_prepare: gpk_padded(N) + gpk_padded(F) must not exceed 65535", X, N, Np, D, P, sf2, Omega, phase, F,
                     W_rand, Yn, Eps, nullptr, S, Coef, ldc, 2, 0,
                     [&](const double* Phi, const double* Wr, double* R, int64_t Cp, int64_t Fp) -> int {
                       GPK_TRY(gpk_gemm(h, GPK_F64, gemm_args(Phi, Fp, 0, Wr, Cp, 1, R, Cp, (int)Np, (int)Cp, (int)Fp, -1.0, 1.0)));
                       return paths_inverse_product(h, W, ldw, Np, Cp, R, R + Np * Cp, R, 1.0);
                     });
}

// the bodies of the single-model entries; grad: the gradient form, which also fills jac
static int paths_step_single(gpk_handle h, bool grad, const double* X, int64_t N, int D, const double* ls, double sf2,
                             const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc, int S, int P,
                             const double* y_mean, const double* y_std, const double* Xq, double* out, double* jac) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Omega && phase && Coef && Xq && out, "paths_step: null pointer");
  GPK_REQUIRE(h, !grad || jac, "paths_step_grad: null jac");
  GPK_TRY(paths_check_single(h, N, D, F, S, P, ldc));
  PathsModel m{X, (int)N, D, sf2, Omega, phase, (int)F, Coef, (long long)ldc, S, P, {}};
  GPK_TRY(paths_fill_k(h, D, P, ls, y_mean, y_std, m.k));
  int rpc = 0, chunks = 0;
  paths_chunks(N + F, S, &rpc, &chunks);
  void* ws = nullptr;
  if (grad) {
    GPK_TRY(gpk_scratch(h, paths_grad_shares(chunks, D, (size_t)S * P) * sizeof(double), &ws));
    return paths_stage_grad(h, m, paths_grad_model(m), Xq, D, nullptr, rpc, chunks, (double*)ws, out, nullptr, nullptr, jac);
  }
  GPK_TRY(gpk_scratch(h, (size_t)chunks * S * P * sizeof(double), &ws));
  return paths_stage(h, m, Xq, D, nullptr, rpc, chunks, (double*)ws, out, nullptr, nullptr);
}

static int paths_rollout_single(gpk_handle h, bool grad, const double* X, int64_t N, int D, const double* ls, double sf2,
                                const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc, int S, int P,
                                const double* y_mean, const double* y_std, const double* x0, int x0_rows, const double* U, int H,
                                const double* lin, double* traj, double* jac) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Omega && phase && Coef && x0 && lin && traj, "paths_rollout: null pointer");
  GPK_REQUIRE(h, !grad || jac, "paths_rollout_grad: null jac");
  GPK_TRY(paths_check_single(h, N, D, F, S, P, ldc));
  GPK_REQUIRE(h, P <= D, "paths_rollout: the state dimension P must not exceed D");
  PathsModel m{X, (int)N, D, sf2, Omega, phase, (int)F, Coef, (long long)ldc, S, P, {}};
  GPK_TRY(paths_fill_k(h, D, P, ls, y_mean, y_std, m.k));
  int rpc = 0, chunks = 0;
  paths_chunks(N + F, S, &rpc, &chunks);
  if (grad) {
    const PathsGradModel g = paths_grad_model(m);
    return paths_rollout_run(h, "paths_rollout", P, D, S, x0, x0_rows, U, H, lin, traj, paths_grad_shares(chunks, D, (size_t)S * P),
                             (size_t)S * P * D, jac,
                             [&](const double* xk, const double* uk, double* partial, const double* d_lin, double* x_next,
                                 double* jac_k) {
                               return paths_stage_grad(h, m, g, xk, P, uk, rpc, chunks, partial, nullptr, d_lin, x_next, jac_k);
                             });
  }
  return paths_rollout_run(h, "paths_rollout", P, D, S, x0, x0_rows, U, H, lin, traj, (size_t)chunks * S * P, 0, nullptr,
                           [&](const double* xk, const double* uk, double* partial, const double* d_lin, double* x_next, double*) {
                             return paths_stage(h, m, xk, P, uk, rpc, chunks, partial, nullptr, d_lin, x_next);
                           });
}

extern "C" int gpk_paths_step(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2, const double* Omega,
                              const double* phase, int64_t F, const double* Coef, int64_t ldc, int S, int P, const double* y_mean,
                              const double* y_std, const double* Xq, double* out) {
  return paths_step_single(h, false, X, N, D, ls, sf2, Omega, phase, F, Coef, ldc, S, P, y_mean, y_std, Xq, out, nullptr);
}

extern "C" int gpk_paths_step_grad(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2,
                                   const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc, int S,
                                   int P, const double* y_mean, const double* y_std, const double* Xq, double* out, double* jac) {
  return paths_step_single(h, true, X, N, D, ls, sf2, Omega, phase, F, Coef, ldc, S, P, y_mean, y_std, Xq, out, jac);
}

extern "C" int gpk_paths_rollout(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2,
                                 const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc, int S, int P,
                                 const double* y_mean, const double* y_std, const double* x0, int x0_rows, const double* U, int H,
                                 const double* lin, double* traj) {
  return paths_rollout_single(h, false, X, N, D, ls, sf2, Omega, phase, F, Coef, ldc, S, P, y_mean, y_std, x0, x0_rows, U, H, lin,
                              traj, nullptr);
}

extern "C" int gpk_paths_rollout_grad(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2,
                                      const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc, int S,
                                      int P, const double* y_mean, const double* y_std, const double* x0, int x0_rows,
                                      const double* U, int H, const double* lin, double* traj, double* jac) {
  return paths_rollout_single(h, true, X, N, D, ls, sf2, Omega, phase, F, Coef, ldc, S, P, y_mean, y_std, x0, x0_rows, U, H, lin,
                              traj, jac);
}

// the bodies of the batch entries; own_z: X is (B x N x D), every model's own basis points (the _z entries); grad: the gradient
// form, which also fills jac
static int paths_step_multi(gpk_handle h, bool own_z, bool grad, const double* X, int64_t N, int D, int B, const double* ls, const double* sf2,
                            const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                            int64_t mstride, int S, const double* shift, const double* scale, const double* Xq, double* out,
                            double* jac) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Omega && phase && Coef && Xq && out, "paths_step_multi: null pointer");
  GPK_REQUIRE(h, !grad || jac, "paths_step_multi_grad: null jac");
  GPK_TRY(paths_check_multi(h, N, D, B, F, S, ldc, mstride));
  PathsMultiModel m{X, own_z, (int)N, D, B, Omega, phase, (int)F, Coef, (long long)ldc, (long long)mstride, S, {}};
  GPK_TRY(paths_fill_multi(h, D, B, ls, sf2, shift, scale, m.k));
  int rpc = 0, chunks = 0;
  paths_chunks(N + F, S, &rpc, &chunks);
  void* ws = nullptr;
  if (grad) {
    GPK_TRY(gpk_scratch(h, paths_grad_shares(chunks, D, (size_t)S * B) * sizeof(double), &ws));
    return paths_stage_multi_grad(h, m, paths_grad_model(m), Xq, D, nullptr, rpc, chunks, (double*)ws, B, out, nullptr, nullptr,
                                  jac);
  }
  GPK_TRY(gpk_scratch(h, (size_t)chunks * S * B * sizeof(double), &ws));
  GPK_TRY(paths_partial_multi(h, m, Xq, D, nullptr, rpc, chunks, (double*)ws));
  hipLaunchKernelGGL(paths_combine_multi_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)B), dim3(256), 0, h->stream,
                     (const double*)ws, chunks, S, B, m.k, out);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

static int paths_rollout_multi(gpk_handle h, bool own_z, bool grad, const double* X, int64_t N, int D, int B, const double* ls,
                               const double* sf2, const double* Omega, const double* phase, int64_t F, const double* Coef,
                               int64_t ldc, int64_t mstride, int S, const double* shift, const double* scale, int nx,
                               const int* coord, const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                               const double* U, int H, const double* lin, double* traj, double* jac) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Omega && phase && Coef && coord && x0 && lin && traj, "paths_rollout_multi: null pointer");
  GPK_REQUIRE(h, !grad || jac, "paths_rollout_multi_grad: null jac");
  GPK_TRY(paths_check_multi(h, N, D, B, F, S, ldc, mstride));
  GPK_REQUIRE(h, nx >= B && nx <= D, "paths_rollout_multi: the state dimension nx must be in [B, D]");
  GPK_REQUIRE(h, (in_shift == nullptr) == (in_scale == nullptr), "paths_rollout_multi: in_shift and in_scale go together");
  PathsMultiModel m{X, own_z, (int)N, D, B, Omega, phase, (int)F, Coef, (long long)ldc, (long long)mstride, S, {}};
  GPK_TRY(paths_fill_multi(h, D, B, ls, sf2, shift, scale, m.k));
  for (int b = 0; b < B; ++b) {
    GPK_REQUIRE(h, coord[b] >= 0 && coord[b] < nx, "paths_rollout_multi: coord must be in [0, nx)");
    GPK_REQUIRE(h, m.k.model_of[coord[b]] < 0, "paths_rollout_multi: coord must be distinct");
    m.k.model_of[coord[b]] = b;
  }
  if (in_shift) {
    GPK_REQUIRE(h, gpk_finite(in_shift, D) && gpk_finite(in_scale, D),
                "paths_rollout_multi: the input scaler must not contain NaN or infinity");
    for (int d = 0; d < D; ++d) {
      GPK_REQUIRE(h, in_scale[d] != 0.0, "paths_rollout_multi: in_scale must be non-zero");
      m.k.in_shift[d] = in_shift[d];
      m.k.in_scale[d] = in_scale[d];
    }
    m.k.scaled = 1;
  }
  int rpc = 0, chunks = 0;
  paths_chunks(N + F, S, &rpc, &chunks);
  const dim3 agrid((unsigned)((S + 255) / 256), (unsigned)nx);
  if (grad) {
    const PathsGradModel g = paths_grad_model(m);
    return paths_rollout_run(h, "paths_rollout_multi", nx, D, S, x0, x0_rows, U, H, lin, traj,
                             paths_grad_shares(chunks, D, (size_t)S * B), (size_t)S * B * D, jac,
                             [&](const double* xk, const double* uk, double* partial, const double* d_lin, double* x_next,
                                 double* jac_k) {
                               return paths_stage_multi_grad(h, m, g, xk, nx, uk, rpc, chunks, partial, nx, nullptr, d_lin, x_next,
                                                             jac_k);
                             });
  }
  return paths_rollout_run(h, "paths_rollout_multi", nx, D, S, x0, x0_rows, U, H, lin, traj, (size_t)chunks * S * B, 0, nullptr,
                           [&](const double* xk, const double* uk, double* partial, const double* d_lin, double* x_next,
                               double*) -> int {
                             GPK_TRY(paths_partial_multi(h, m, xk, nx, uk, rpc, chunks, partial));
                             hipLaunchKernelGGL(paths_advance_multi_kernel, agrid, dim3(256), 0, h->stream, (const double*)partial,
                                                chunks, S, B, nx, D, m.k, xk, uk, d_lin, x_next);
                             GPK_LAUNCH_CHECK(h);
                             return GPK_OK;
                           });
}

extern "C" int gpk_paths_step_multi(gpk_handle h, const double* X, int64_t N, int D, int B, const double* ls, const double* sf2,
                                    const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                                    int64_t mstride, int S, const double* shift, const double* scale, const double* Xq,
                                    double* out) {
  return paths_step_multi(h, false, false, X, N, D, B, ls, sf2, Omega, phase, F, Coef, ldc, mstride, S, shift, scale, Xq, out, nullptr);
}

extern "C" int gpk_paths_rollout_multi(gpk_handle h, const double* X, int64_t N, int D, int B, const double* ls, const double* sf2,
                                       const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                                       int64_t mstride, int S, const double* shift, const double* scale, int nx, const int* coord,
                                       const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                       const double* U, int H, const double* lin, double* traj) {
  return paths_rollout_multi(h, false, false, X, N, D, B, ls, sf2, Omega, phase, F, Coef, ldc, mstride, S, shift, scale, nx, coord,
                             in_shift, in_scale, x0, x0_rows, U, H, lin, traj, nullptr);
}

// ---- the sparse models: every model has its own basis points (its inducing inputs) -------------------------------------------
extern "C" int gpk_paths_step_multi_z(gpk_handle h, const double* Zs, int64_t N, int D, int B, const double* ls, const double* sf2,
                                      const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                                      int64_t mstride, int S, const double* shift, const double* scale, const double* Xq,
                                      double* out) {
  return paths_step_multi(h, true, false, Zs, N, D, B, ls, sf2, Omega, phase, F, Coef, ldc, mstride, S, shift, scale, Xq, out, nullptr);
}

extern "C" int gpk_paths_rollout_multi_z(gpk_handle h, const double* Zs, int64_t N, int D, int B, const double* ls,
                                         const double* sf2, const double* Omega, const double* phase, int64_t F, const double* Coef,
                                         int64_t ldc, int64_t mstride, int S, const double* shift, const double* scale, int nx,
                                         const int* coord, const double* in_shift, const double* in_scale, const double* x0,
                                         int x0_rows, const double* U, int H, const double* lin, double* traj) {
  return paths_rollout_multi(h, true, false, Zs, N, D, B, ls, sf2, Omega, phase, F, Coef, ldc, mstride, S, shift, scale, nx, coord,
                             in_shift, in_scale, x0, x0_rows, U, H, lin, traj, nullptr);
}

// ---- the gradient forms of the four batch entries ------------------------------------------------------------------------------
#define GPK_PATHS_MULTI_GRAD(SUFFIX, OWNZ)                                                                                     \
  extern "C" int gpk_paths_step_multi_grad##SUFFIX(gpk_handle h, const double* X, int64_t N, int D, int B, const double* ls,   \
                                                   const double* sf2, const double* Omega, const double* phase, int64_t F,     \
                                                   const double* Coef, int64_t ldc, int64_t mstride, int S,                    \
                                                   const double* shift, const double* scale, const double* Xq, double* out,    \
                                                   double* jac) {                                                              \
    return paths_step_multi(h, OWNZ, true, X, N, D, B, ls, sf2, Omega, phase, F, Coef, ldc, mstride, S, shift, scale, Xq, out, \
                            jac);                                                                                              \
  }                                                                                                                            \
  extern "C" int gpk_paths_rollout_multi_grad##SUFFIX(                                                                         \
      gpk_handle h, const double* X, int64_t N, int D, int B, const double* ls, const double* sf2, const double* Omega,        \
      const double* phase, int64_t F, const double* Coef, int64_t ldc, int64_t mstride, int S, const double* shift,            \
      const double* scale, int nx, const int* coord, const double* in_shift, const double* in_scale, const double* x0,         \
      int x0_rows, const double* U, int H, const double* lin, double* traj, double* jac) {                                     \
    return paths_rollout_multi(h, OWNZ, true, X, N, D, B, ls, sf2, Omega, phase, F, Coef, ldc, mstride, S, shift, scale, nx,   \
                               coord, in_shift, in_scale, x0, x0_rows, U, H, lin, traj, jac);                                  \
  }
GPK_PATHS_MULTI_GRAD(, false)
GPK_PATHS_MULTI_GRAD(_z, true)
#undef GPK_PATHS_MULTI_GRAD

// The set-up of a sparse model's path set (gpk_sparse_paths_prepare, gpk_sparse.hip, which takes the model apart): Z (m x D),
// the inverse factors Wuu and WS (mp x mp, lower tiles) and alpha_u (m x P) are the assembled model's.
int gpk_paths_prepare_two(gpk_handle h, const double* Z, int64_t m, int D, int P, double sf2, const double* Wuu, const double* WS,
                          int64_t mp, const double* alpha, const double* Omega, const double* phase, int64_t F,
                          const double* W_rand, const double* Xi, int S, double* Coef, int64_t ldc, double* Zdst) {
  GPK_REQUIRE(h, Omega && phase && W_rand && Xi && Coef && Zdst, "sparse_paths_prepare: null pointer");
  GPK_TRY(paths_check_single(h, m, D, F, S, P, ldc));
  // areas: Xp = Xi, T, R.  R = Phi_Z Wr; R <- -Wuu^T (Wuu R); R += WS^T Xp (k >= row-tile start).  Phi_Z and Xp are zero in the
  // padding rows and both factors are block diagonal there (the identity), so the padding rows of every product are exact zeros
  // and nothing of the padding reaches a row below m.
  return paths_setup(h, "sparse_paths_prepare: gpk_padded(m) + gpk_padded(F) must not exceed 65535", Z, m, mp, D, P, sf2, Omega,
                     phase, F, W_rand, nullptr, Xi, alpha, S, Coef, ldc, 3, 2,
                     [&](const double* Phi, const double* Wr, double* Xp, int64_t Cp, int64_t Fp) -> int {
                       double* T = Xp + mp * Cp;
                       double* R = T + mp * Cp;
                       GPK_CHECK_HIP(h, hipMemcpyAsync(Zdst, Z, (size_t)m * D * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
                       GPK_TRY(gpk_gemm(h, GPK_F64, gemm_args(Phi, Fp, 0, Wr, Cp, 1, R, Cp, (int)mp, (int)Cp, (int)Fp, 1.0, 0.0)));
                       GPK_TRY(paths_inverse_product(h, Wuu, mp, mp, Cp, R, T, R, -1.0));
                       GemmArgs g3 = gemm_args(WS, mp, 1, Xp, Cp, 1, R, Cp, (int)mp, (int)Cp, (int)mp, 1.0, 1.0);
                       g3.kb_row = GPK_TILE;
                       return gpk_gemm(h, GPK_F64, g3);
                     });
}
