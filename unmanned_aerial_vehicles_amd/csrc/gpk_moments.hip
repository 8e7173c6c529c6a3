// Exact moment matching (K11, method "moment"): mean, covariance and input-output covariance of the posterior of [C.]RBF[+White]
// models at a GAUSSIAN query z ~ N(m, S), in closed form (Girard; Quinonero-Candela; Deisenroth), and the horizon chain built on it.
// S is non-zero only in the nx x nx state block; all of it in normalised model units, nu_i = x_i - m, Lam_b = diag(ls_b^2), P_b = 1 / Lam_b:
//
//   l_i        = sf2_b |I + S P_b|^(-1/2) exp(-nu_i^T (S + Lam_b)^-1 nu_i / 2)
//   E[mu_b]    = sum_i alpha_i l_i,            Cov[z, mu_b] = S (S + Lam_b)^-1 sum_i alpha_i l_i nu_i
//   pair (a, b):  T = S_x + diag(1 / (P_a + P_b)) = C C^T,  M = S_x T^-1 diag(1 / (P_a + P_b)) = G G^T  (= R^-1 S with R = S (P_a + P_b) + I),
//                 log |R| = log |T| + sum log (P_a + P_b)
//   w_i^a      = G^T (P_a nu_i^a)_x,           lam_i^a = log sf2_a - nu_i^a^T P_a nu_i^a / 2 + |w_i^a|^2 / 2
//   L_ij       = exp(-log|R| / 2 + lam_i^a + lam_j^b + w_i^a . w_j^b)         one exp per pair of rows, never stored
//   E[mu_a mu_b] = sum_ij alpha_i^a alpha_j^b L_ij,     E[v_b] = kss_b - sum_ij (K_b^-1)_ij L^bb_ij
//   V_ab       = E[mu_a mu_b] - E[mu_a] E[mu_b] + [a == b] (max(E[v_b], floor) [+ noise])
//
// Five launches per batch of R <= 32 Gaussian queries (the rows of a predict_moments call, or the rollouts of one stage of the chain):
//   moments_setup_kernel     one wave per (query, model or pair): the sequential nx <= 16 factorisations
//   moments_row_*_kernel     the N rows: l_i and the workgroups' shares of E[mu] and sum alpha l nu;  lam_i, w_i per (pair, side)
//   moments_pair_kernel<P>   the N x N pairs in 64 x 64 tiles (a == b: the lower tiles, the others counted twice): every K^-1 and alpha
//                            tile is read ONCE and serves all R queries; the tile's sums are added in a fixed order in LDS and then to
//                            the workgroup's own slot - no atomics; workgroup g owns tiles g, g + G, ..; where G U leaves the
//                            card idle (the sparse sizes, small exact models) the R queries are cut into groups, a third grid
//                            dimension: workgroup (g, u, zq) walks the same tiles for its own queries and re-reads the tile
//   moments_finish_kernel    one workgroup per query: the slots added in workgroup order, V, the raw units and - in the chain - the
//                            stage:  x+ = x + lin q + E E[mu],  Sigma+ = A0 Sigma A0^T + A0 Cx E^T + E Cx^T A0^T + E V E^T + Q  with
//                            A0 = I + lin[:, :nx] and Cx the state rows of the raw input-output covariance; the lower triangle is formed
//                            and mirrored.
// Nothing depends on R or on the other queries: query r of a batch has the bits of the same query served alone.
#include "gpk_horizon.h"

namespace {

constexpr int MM_TILE = 64;        // rows and columns of a pair tile; a thread holds 4 x 4 pairs
constexpr int MM_CH = 12;          // tile sums reduced per pass through LDS
constexpr int MM_MAXG = 512;       // workgroups per pair at most (two per CU)
constexpr int MM_WS = 17;          // doubles per row of the row pass: w (16) and lam
constexpr int MM_ROWS = 256;       // rows per workgroup of the row pass

struct MomK {
  int B, P, D, nx, NO, U;            // models, outputs per model, query width, state width, B * P, pairs B (B + 1) / 2
  long long N, Np, ldk;
  const double* X[GPK_SMALL_MAX_MODELS];
  const double* alpha[GPK_SMALL_MAX_MODELS];
  const double* Kinv[GPK_SMALL_MAX_MODELS];
  double ls[GPK_SMALL_MAX_MODELS][16], lsf2[GPK_SMALL_MAX_MODELS], kss[GPK_SMALL_MAX_MODELS], noise[GPK_SMALL_MAX_MODELS];
  double ymean[16], ystd[16];        // per output, the output scaler folded in
  double in_shift[16], in_scale[16];
  double floor_;
  int add_noise, scaled;
  int model_of[16];                  // state coordinate -> output, or -1
};

__device__ __forceinline__ void pair_of(int u, int& a, int& b) {
  a = 0;
  while ((a + 1) * (a + 2) / 2 <= u) ++a;
  b = u - a * (a + 1) / 2;
}

// In-place lower Cholesky factor of the leading n x n block, one wave, row `lane` owned by that lane.  A pivot that is not
// positive gives a zero column (semi-definite M: what Sigma = 0 or a rank-deficient Sigma produces).
__device__ __forceinline__ void mm_chol(double (*A)[17], int n, int lane) {
  for (int c = 0; c < n; ++c) {
    __syncthreads();
    const double p = A[c][c];
    const double d = p > 0.0 ? sqrt(p) : 0.0;
    __syncthreads();
    if (lane == c) A[c][c] = d;
    if (lane > c && lane < n) A[lane][c] = p > 0.0 ? A[lane][c] / d : 0.0;
    __syncthreads();
    if (lane > c && lane < n)
      for (int j = c + 1; j <= lane; ++j) A[lane][j] -= A[lane][c] * A[j][c];
  }
  __syncthreads();
}

// grid (R, B + U), 64 threads.  Units [0, B): model b -> Bm = (S_x + Lam_b,x)^-1 and cm = log sf2_b - log|I + S P_b| / 2; unit 0 also
// writes S_z.  Units [B, B + U): pair u -> G (lower, zero above) and cl = -log|R| / 2.  Sraw: R x nx x nx raw covariances.
__global__ __launch_bounds__(64) void moments_setup_kernel(MomK k, const double* __restrict__ Sraw, double* Sz, double* Bm, double* cm,
                                                           double* G, double* cl) {
  __shared__ double S[16][17], T[16][17], Ci[16][17], Y[16][17], dd[16];
  const int lane = threadIdx.x, r = blockIdx.x, unit = blockIdx.y, nx = k.nx;
  for (int e = lane; e < 256; e += 64) {
    const int i = e >> 4, j = e & 15;
    double s = 0.0;
    if (i < nx && j < nx) {
      s = Sraw[((long long)r * nx + i) * nx + j];
      if (k.scaled) s = s / (k.in_scale[i] * k.in_scale[j]);
    }
    S[i][j] = s;
    Ci[i][j] = 0.0;
    Y[i][j] = 0.0;
  }
  int a = 0, b = 0;
  const bool pair = unit >= k.B;
  if (pair) pair_of(unit - k.B, a, b); else a = b = unit;
  if (lane < 16) {
    double d = 1.0;
    if (lane < nx) {
      const double la = k.ls[a][lane], lb = k.ls[b][lane];
      d = pair ? 1.0 / (1.0 / (la * la) + 1.0 / (lb * lb)) : la * la;
    }
    dd[lane] = d;
  }
  __syncthreads();
  for (int e = lane; e < 256; e += 64) {
    const int i = e >> 4, j = e & 15;
    T[i][j] = S[i][j] + (i == j ? dd[i] : 0.0);
  }
  if (unit == 0)
    for (int e = lane; e < 256; e += 64) Sz[(long long)r * 256 + e] = S[e >> 4][e & 15];
  mm_chol(T, nx, lane);
  // Ci = C^-1, lane j solves column j
  if (lane < nx) {
    const int j = lane;
    for (int i = j; i < nx; ++i) {
      double s = i == j ? 1.0 : 0.0;
      for (int c = j; c < i; ++c) s -= T[i][c] * Ci[c][j];
      Ci[i][j] = s / T[i][i];
    }
  }
  __syncthreads();
  double logdet = 0.0;
  for (int c = 0; c < nx; ++c) logdet += 2.0 * log(T[c][c]) - log(dd[c]);
  if (!pair) {
    // Bm = Ci^T Ci, the lower triangle formed and mirrored
    for (int e = lane; e < 256; e += 64) {
      const int i = e >> 4, j = e & 15;
      if (i < nx && j <= i) {
        double s = 0.0;
        for (int c = i; c < nx; ++c) s = __builtin_fma(Ci[c][i], Ci[c][j], s);
        Y[i][j] = s;
        Y[j][i] = s;
      }
    }
    __syncthreads();
    double* o = Bm + ((long long)r * k.B + unit) * 256;
    for (int e = lane; e < 256; e += 64) o[e] = Y[e >> 4][e & 15];
    if (lane == 0) cm[(long long)r * k.B + unit] = k.lsf2[unit] - 0.5 * logdet;
    return;
  }
  // Y = Ci S;  M = Y^T Ci diag(dd) (lower triangle, mirrored) -> T;  G = chol(M)
  for (int e = lane; e < 256; e += 64) {
    const int i = e >> 4, j = e & 15;
    if (i < nx && j < nx) {
      double s = 0.0;
      for (int c = 0; c <= i; ++c) s = __builtin_fma(Ci[i][c], S[c][j], s);
      Y[i][j] = s;
    }
  }
  __syncthreads();
  for (int e = lane; e < 256; e += 64) {
    const int i = e >> 4, j = e & 15;
    if (i < nx && j <= i) {
      double s = 0.0;
      for (int c = j; c < nx; ++c) s = __builtin_fma(Y[c][i], Ci[c][j], s);
      s *= dd[j];
      T[i][j] = s;
      T[j][i] = s;
    }
  }
  mm_chol(T, nx, lane);
  const int u = unit - k.B;
  double* o = G + ((long long)r * k.U + u) * 256;
  for (int e = lane; e < 256; e += 64) {
    const int i = e >> 4, j = e & 15;
    o[e] = (i < nx && j <= i) ? T[i][j] : 0.0;
  }
  if (lane == 0) cl[(long long)r * k.U + u] = -0.5 * logdet;
}

// grid (ceil(N / 256), R, B), 256 threads.  q: R x D scaled queries.  part[((wg R + r) B + b) P + p][17]: entries d < nx the share of
// sum_i alpha_ip l_i nu_id, entry 16 that of sum_i alpha_ip l_i; the rows of a workgroup are added in row order.
__global__ __launch_bounds__(256) void moments_row_mean_kernel(MomK k, const double* __restrict__ q, const double* __restrict__ Bm,
                                                               const double* __restrict__ cm, double* part) {
  __shared__ double sB[16][17], lv[MM_ROWS][MM_WS], z[16], ils2[16];
  const int tid = threadIdx.x, r = blockIdx.y, b = blockIdx.z, R = gridDim.y, D = k.D, nx = k.nx, P = k.P;
  const long long row = (long long)blockIdx.x * MM_ROWS + tid;
  sB[tid >> 4][tid & 15] = Bm[((long long)r * k.B + b) * 256 + tid];
  if (tid < 16) {
    z[tid] = tid < D ? q[(long long)r * D + tid] : 0.0;
    ils2[tid] = (tid >= nx && tid < D) ? 1.0 / (k.ls[b][tid] * k.ls[b][tid]) : 0.0;
  }
  __syncthreads();
  const bool live = row < k.N;
  const double* xr = k.X[b] + row * D;
  double nu[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) nu[d] = (live && d < D) ? xr[d] - z[d] : 0.0;
  double quad = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i < nx) {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) t = __builtin_fma(sB[i][j], nu[j], t);      // (columns >= nx of Bm are zero)
      quad = __builtin_fma(nu[i], t, quad);
    } else {
      quad = __builtin_fma(nu[i] * nu[i], ils2[i], quad);
    }
  }
  const double l = live ? exp(cm[(long long)r * k.B + b] - 0.5 * quad) : 0.0;
#pragma unroll
  for (int d = 0; d < 16; ++d) lv[tid][d] = l * nu[d];
  lv[tid][16] = l;
  __syncthreads();
  const long long base = (long long)blockIdx.x * MM_ROWS;
  for (int e = tid; e < P * MM_WS; e += 256) {
    const int p = e / MM_WS, d = e % MM_WS;
    if (d >= nx && d != 16) continue;
    double s = 0.0;
    for (int t = 0; t < MM_ROWS; ++t) {
      const double al = base + t < k.N ? k.alpha[b][(base + t) * P + p] : 0.0;
      s = __builtin_fma(al, lv[t][d], s);
    }
    part[((((long long)blockIdx.x * R + r) * k.B + b) * P + p) * MM_WS + d] = s;
  }
}

// grid (ceil(N / 256), R, 2 U), 256 threads.  rowq[((a a + 2 b + side) R + r) Np + i][17] = w_i (entries < nx, zero to 16) and lam_i of
// model a (side 0) or b (side 1) of pair u; a == b has side 0 alone.
__global__ __launch_bounds__(256) void moments_row_pair_kernel(MomK k, const double* __restrict__ q, const double* __restrict__ G,
                                                               double* rowq) {
  __shared__ double sG[16][17], z[16], ip[16];
  const int tid = threadIdx.x, r = blockIdx.y, u = blockIdx.z >> 1, side = blockIdx.z & 1, R = gridDim.y, D = k.D, nx = k.nx;
  int a, b;
  pair_of(u, a, b);
  if (side == 1 && a == b) return;
  const int m = side ? b : a;
  const long long row = (long long)blockIdx.x * MM_ROWS + tid;
  sG[tid >> 4][tid & 15] = G[((long long)r * k.U + u) * 256 + tid];
  if (tid < 16) {
    z[tid] = tid < D ? q[(long long)r * D + tid] : 0.0;
    ip[tid] = tid < D ? 1.0 / (k.ls[m][tid] * k.ls[m][tid]) : 0.0;
  }
  __syncthreads();
  if (row >= k.N) return;
  const double* xr = k.X[m] + row * D;
  double t[16];
  double e0 = 0.0;
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    const double nu = d < D ? xr[d] - z[d] : 0.0;
    t[d] = nu * ip[d];
    e0 = __builtin_fma(nu, t[d], e0);
  }
  double* o = rowq + (((long long)(a * a + 2 * b + side) * R + r) * k.Np + row) * MM_WS;
  double ww = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    double w = 0.0;
    if (c < nx) {
#pragma unroll
      for (int i = c; i < 16; ++i) w = __builtin_fma(sG[i][c], t[i], w);       // (rows >= nx of G are zero)
    }
    o[c] = w;
    ww = __builtin_fma(w, w, ww);
  }
  o[16] = k.lsf2[m] - 0.5 * e0 + 0.5 * ww;
}

// grid (G, U, NQ), 256 threads: thread (ty, tx) = (tid >> 4, tid & 15) holds the pairs (ty + 16 ii, tx + 16 jj) of a tile.
// part[((u G + g) R + r) NV + v], NV = 1 + P (P + 1) / 2: v = 0 the K^-1 sum (a == b), v = 1 + p (p + 1) / 2 + q the alpha sums.
// Workgroup (g, u, zq) serves the queries [zq R / NQ, (zq + 1) R / NQ) on the tiles g, g + G, ..: a slot (g, r) is written by one
// workgroup, over the same tiles in the same order whatever NQ is - the split changes no bit; it costs one more read of the
// tile of K^-1 (of Q, for a sparse model) and of the alpha tiles per group, outside the query loop as before.  SPLIT = false is
// the kernel without the dimension (NQ = 1: grid (G, U), every query), instruction for instruction what the large exact shapes
// have always run - measured, the general loop bounds alone cost those shapes 1 % (profiles/r28_exp_sparse_moments.log).
template <int P, bool SPLIT>
__global__ __launch_bounds__(256) void moments_pair_kernel(MomK k, int R, const double* __restrict__ rowq,
                                                           const double* __restrict__ cl, double* part) {
  constexpr int NV = 1 + P * (P + 1) / 2;
  __shared__ double sA[MM_TILE][P], sB[MM_TILE][P], sWa[MM_TILE][MM_WS], sWb[MM_TILE][MM_WS], red[MM_CH][16 * 17], red2[MM_CH][16];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, u = blockIdx.y, g = blockIdx.x, G_ = gridDim.x, nx = k.nx;
  const int r0 = SPLIT ? (int)(blockIdx.z * (unsigned)R / gridDim.z) : 0;      // (R, NQ <= 32)
  const int r1 = SPLIT ? (int)((blockIdx.z + 1) * (unsigned)R / gridDim.z) : R;
  int a, b;
  pair_of(u, a, b);
  const bool same = a == b;
  const long long N = k.N;
  const int nt = (int)((N + MM_TILE - 1) / MM_TILE);
  const long long ntiles = same ? (long long)nt * (nt + 1) / 2 : (long long)nt * nt;
  const double* Wa = rowq + (long long)(a * a + 2 * b) * R * k.Np * MM_WS;      // (pair, side) -> slot a a + 2 b + side: B B slots
  const double* Wb = same ? Wa : Wa + (long long)R * k.Np * MM_WS;
  bool first = true;
  for (long long t = g; t < ntiles; t += G_) {
    int ti, tj;
    if (same) {
      ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
      while ((long long)(ti + 1) * (ti + 2) / 2 <= t) ++ti;
      while ((long long)ti * (ti + 1) / 2 > t) --ti;
      tj = (int)(t - (long long)ti * (ti + 1) / 2);
    } else {
      ti = (int)(t / nt);
      tj = (int)(t % nt);
    }
    const bool sym = same && ti != tj;
    const double wgt = sym ? 2.0 : 1.0;
    const long long i0 = (long long)ti * MM_TILE, j0 = (long long)tj * MM_TILE;
    double kv[4][4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const long long i = i0 + ty + 16 * ii, j = j0 + tx + 16 * jj;
        // the lower triangle of K^-1 is the matrix; rows and columns >= N (its identity padding) are masked
        kv[ii][jj] = (same && i < N && j < N) ? k.Kinv[a][(i > j ? i : j) * k.ldk + (i > j ? j : i)] : 0.0;
      }
    __syncthreads();
    for (int e = tid; e < MM_TILE * P; e += 256) {
      const int row = e / P, p = e % P;
      sA[row][p] = i0 + row < N ? k.alpha[a][(i0 + row) * P + p] : 0.0;
      sB[row][p] = j0 + row < N ? k.alpha[b][(j0 + row) * P + p] : 0.0;
    }
    for (int r = r0; r < r1; ++r) {
      __syncthreads();
      for (int e = tid; e < MM_TILE * MM_WS; e += 256) {
        const int row = e / MM_WS;
        sWa[row][e % MM_WS] = i0 + row < N ? Wa[((long long)r * k.Np + i0) * MM_WS + e] : 0.0;
        sWb[row][e % MM_WS] = j0 + row < N ? Wb[((long long)r * k.Np + j0) * MM_WS + e] : 0.0;
      }
      __syncthreads();
      const double c0 = cl[(long long)r * k.U + u];
      double ex[4][4];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) ex[ii][jj] = (c0 + sWa[ty + 16 * ii][16]) + sWb[tx + 16 * jj][16];
      for (int c = 0; c < nx; ++c) {
        double wa[4], wb[4];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) { wa[ii] = sWa[ty + 16 * ii][c]; wb[ii] = sWb[tx + 16 * ii][c]; }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) ex[ii][jj] = __builtin_fma(wa[ii], wb[jj], ex[ii][jj]);
      }
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const bool live = i0 + ty + 16 * ii < N && j0 + tx + 16 * jj < N;
          ex[ii][jj] = live ? exp(ex[ii][jj]) : 0.0;
        }
      // the tile's sums, MM_CH at a time: every thread's share to LDS, 16 shares per lane group in lane order, the 16 groups in
      // group order, then thread v adds the sum to the workgroup's slot
      double* slot = part + (((long long)u * G_ + g) * R + r) * NV;
      auto flush = [&](int chunk, int nvals) {
        __syncthreads();
        if (ty < nvals) {
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < 16; ++c) s += red[ty][tx * 17 + c];
          red2[ty][tx] = s;
        }
        __syncthreads();
        if (tid < nvals) {
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < 16; ++c) s += red2[tid][c];
          s *= wgt;
          double* dst = slot + chunk * MM_CH + tid;
          *dst = first ? s : *dst + s;
        }
      };
      auto emit = [&](int v, double x) {
        red[v % MM_CH][ty * 17 + tx] = x;
        if (v % MM_CH == MM_CH - 1 || v == NV - 1) flush(v / MM_CH, v % MM_CH + 1);
      };
      {
        double s = 0.0;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) s = __builtin_fma(ex[ii][jj], kv[ii][jj], s);
        emit(0, s);
      }
      double uu[4][P];
#pragma unroll
      for (int qq = 0; qq < P; ++qq) {
        double bj[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) bj[jj] = sB[tx + 16 * jj][qq];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          double s = 0.0;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) s = __builtin_fma(ex[ii][jj], bj[jj], s);
          uu[ii][qq] = s;
        }
      }
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int qq = 0; qq <= p; ++qq) {
          double s = 0.0;
#pragma unroll
          for (int ii = 0; ii < 4; ++ii) s = __builtin_fma(sA[ty + 16 * ii][p], uu[ii][qq], s);
          if (sym) {      // an off-diagonal tile stands for its mirror image too: alpha_ip alpha_jq + alpha_iq alpha_jp
            double s2 = 0.0;
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) s2 = __builtin_fma(sA[ty + 16 * ii][qq], uu[ii][p], s2);
            s = 0.5 * (s + s2);      // (the slot takes the sum times wgt = 2)
          }
          emit(1 + p * (p + 1) / 2 + qq, s);
        }
    }
    first = false;
  }
}

// grid R, 256 threads, thread (i, j) = (tid >> 4, tid & 15).  v.out: mean (R x NO), cov (R x NO x NO), xcov (R x NO x D) in raw
// units, null where not wanted.  Past the moments the launch composes the stage of the chain (gpk_horizon.h; v.x null: a
// predict_moments call, outputs only).
__global__ __launch_bounds__(256) void moments_finish_kernel(MomK k, StageView v, int R, int G_, int nrw, int NV,
                                                             const double* __restrict__ Sz, const double* __restrict__ Bm,
                                                             const double* __restrict__ rowpart, const double* __restrict__ pairpart) {
  double *omean = v.out[0], *ocov = v.out[1], *oxcov = v.out[2];
  __shared__ double Em[16], Cz[16][17], Tm[16][17], Vr[16][17], Cx[16][17], sS[16][17], pv[160];
  __shared__ double A[16][17], Sg[16][17], T[16][17], F[16][17], q[16], xn[16], mu[16];
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, r = blockIdx.x;
  const int nx = k.nx, D = k.D, NO = k.NO, P = k.P, B = k.B;
  sS[i][j] = Sz[(long long)r * 256 + tid];
  for (int e = tid; e < NO * MM_WS; e += 256) {
    const int o = e / MM_WS, d = e % MM_WS;
    if (d >= nx && d != 16) continue;
    double s = 0.0;
    for (int w = 0; w < nrw; ++w) s += rowpart[(((long long)w * R + r) * NO + o) * MM_WS + d];
    if (d == 16) Em[o] = s; else Cz[o][d] = s;
  }
  for (int e = tid; e < k.U * NV; e += 256) {
    const int u = e / NV, vv = e % NV;
    const double* p = pairpart + ((long long)u * G_ * R + r) * NV + vv;
    double s = 0.0;
#pragma unroll 8
    for (int g = 0; g < G_; ++g) s += p[(long long)g * R * NV];
    pv[e] = s;
  }
  __syncthreads();
  // V in raw units, the lower triangle formed and mirrored
  if (i < NO && j <= i) {
    const int u = B > 1 ? i * (i + 1) / 2 + j : 0;
    const int at = B > 1 ? u * NV + 1 : 1 + i * (i + 1) / 2 + j;
    double s = pv[at] - Em[i] * Em[j];
    if (i == j) {
      const int b = B > 1 ? i : 0;
      const double ev = k.kss[b] - pv[B > 1 ? u * NV : 0];
      double var = ev > k.floor_ ? ev : k.floor_;
      if (k.add_noise) var += k.noise[b];
      s += var;
    }
    s *= k.ystd[i] * k.ystd[j];
    Vr[i][j] = s;
    Vr[j][i] = s;
  }
  // Cov[z, mu_o] = S_z Bm_b (sum alpha l nu_x): Tm = Bm_b Cz[o], then S_z Tm
  if (i < NO && j < nx) {
    const double* bm = Bm + ((long long)r * B + i / P) * 256;
    double s = 0.0;
    for (int c = 0; c < nx; ++c) s = __builtin_fma(bm[j * 16 + c], Cz[i][c], s);
    Tm[i][j] = s;
  }
  __syncthreads();
  if (i < NO && j < nx) {
    double s = 0.0;
    for (int c = 0; c < nx; ++c) s = __builtin_fma(sS[j][c], Tm[i][c], s);
    Cx[i][j] = k.ystd[i] * (k.scaled ? k.in_scale[j] * s : s);
  }
  if (tid < NO) mu[tid] = k.ymean[tid] + k.ystd[tid] * Em[tid];
  __syncthreads();
  if (omean && tid < NO) omean[(long long)r * NO + tid] = mu[tid];
  if (ocov && i < NO && j < NO) ocov[((long long)r * NO + i) * NO + j] = Vr[i][j];
  if (oxcov && i < NO && j < D) oxcov[((long long)r * NO + i) * D + j] = j < nx ? Cx[i][j] : 0.0;
  if (!v.x) return;
  stage_load(v, nx, D, r, tid, q, Sg);
  if (i < nx && j < nx) A[i][j] = (i == j ? 1.0 : 0.0) + v.lin[i * D + j];
  __syncthreads();
  stage_mean(v, k.model_of, nx, D, tid, q, mu, xn);
  stage_left(nx, tid, A, Sg, T);
  if (i < nx && j < nx) {
    // F = A0 Cx E^T: column j is A0 times the input-output covariance of the output that drives coordinate j
    const int o = k.model_of[j];
    double f = 0.0;
    if (o >= 0)
      for (int c = 0; c < nx; ++c) f = __builtin_fma(A[i][c], Cx[o][c], f);
    F[i][j] = f;
  }
  __syncthreads();
  stage_right(v, nx, r, tid, T, A, [&](double s, int a, int b) {
    s += F[a][b] + F[b][a];
    const int oa = k.model_of[a], ob = k.model_of[b];
    return oa >= 0 && ob >= 0 ? s + Vr[oa][ob] : s;
  });
  stage_store(v, k.scaled, k.in_shift, k.in_scale, nx, D, r, tid, xn);
}

// The device work area of one batch of R queries, carved from `base`.
struct MomWork {
  double *Sz, *Bm, *cm, *G, *cl, *rowq, *rowpart, *pairpart;
  int nrw, G_, NV, NQ;
  size_t doubles;
};
// groups of queries of the pair launch: as many as bring G U workgroups to two per CU and no more, at most R; one from G U = 512 on
// (the large exact shapes: the launch as it always was).  Option moments_query_groups = n >= 1 caps the count (1: no split).
int mm_query_groups(gpk_handle h, long long wgs, int R) {
  if (wgs >= MM_MAXG) return 1;
  long long nq = 2ll * gpk_cus(h) / wgs;
  if (h->moments_query_groups >= 1 && nq > h->moments_query_groups) nq = h->moments_query_groups;
  return (int)(nq < 1 ? 1 : nq > R ? R : nq);
}

MomWork mm_work(gpk_handle h, const MomK& k, int R, double* base) {
  MomWork w{};
  const int nt = (int)((k.N + MM_TILE - 1) / MM_TILE);
  const long long lower = (long long)nt * (nt + 1) / 2;
  w.nrw = (int)((k.N + MM_ROWS - 1) / MM_ROWS);
  w.G_ = (int)(lower < MM_MAXG ? lower : MM_MAXG);
  w.NV = 1 + k.P * (k.P + 1) / 2;
  w.NQ = mm_query_groups(h, (long long)w.G_ * k.U, R);
  size_t at = 0;
  auto take = [&](size_t n) { double* p = base ? base + at : nullptr; at += n; return p; };
  w.Sz = take((size_t)R * 256);
  w.Bm = take((size_t)R * k.B * 256);
  w.cm = take((size_t)R * k.B);
  w.G = take((size_t)R * k.U * 256);
  w.cl = take((size_t)R * k.U);
  w.rowq = take((size_t)k.B * k.B * R * k.Np * MM_WS);      // one slot per (pair, side) in use: a == b has side 0 alone
  w.rowpart = take((size_t)w.nrw * R * k.NO * MM_WS);
  w.pairpart = take((size_t)k.U * w.G_ * R * w.NV);
  w.doubles = at;
  return w;
}

template <int P>
void mm_pair_launch(gpk_handle h, const MomK& k, const MomWork& w, int R) {
  if (w.NQ > 1)
    hipLaunchKernelGGL((moments_pair_kernel<P, true>), dim3((unsigned)w.G_, (unsigned)k.U, (unsigned)w.NQ), dim3(256), 0, h->stream, k,
                       R, (const double*)w.rowq, (const double*)w.cl, w.pairpart);
  else
    hipLaunchKernelGGL((moments_pair_kernel<P, false>), dim3((unsigned)w.G_, (unsigned)k.U), dim3(256), 0, h->stream, k, R,
                       (const double*)w.rowq, (const double*)w.cl, w.pairpart);
}

// The four launches ahead of the finishing one: d_q (R x D scaled queries) and d_S (R x nx x nx raw covariances) on the device.
int mm_launch(gpk_handle h, const MomK& k, const MomWork& w, int R, const double* d_q, const double* d_S) {
  if (h->gram_log)   // option gram_log = 1: the form this batch's launches take (the tests assert it per case)
    fprintf(stderr, "GPKMM fwd %d %d %d %d %lld %d cus%d g%d u%d nq%d split%d nrw%d nv%d p%d\n", k.B, k.P, k.D, k.nx, k.N, R, gpk_cus(h),
            w.G_, k.U, w.NQ, w.NQ > 1 ? 1 : 0, w.nrw, w.NV, k.P);
  hipLaunchKernelGGL(moments_setup_kernel, dim3((unsigned)R, (unsigned)(k.B + k.U)), dim3(64), 0, h->stream, k, d_S, w.Sz, w.Bm, w.cm,
                     w.G, w.cl);
  GPK_LAUNCH_CHECK(h);
  hipLaunchKernelGGL(moments_row_mean_kernel, dim3((unsigned)w.nrw, (unsigned)R, (unsigned)k.B), dim3(256), 0, h->stream, k, d_q,
                     (const double*)w.Bm, (const double*)w.cm, w.rowpart);
  hipLaunchKernelGGL(moments_row_pair_kernel, dim3((unsigned)w.nrw, (unsigned)R, (unsigned)(2 * k.U)), dim3(256), 0, h->stream, k, d_q,
                     (const double*)w.G, w.rowq);
  GPK_LAUNCH_CHECK(h);
  switch (k.P) {
#define GPK_MM_CASE(p) case p: mm_pair_launch<p>(h, k, w, R); break;
    GPK_MM_CASE(1) GPK_MM_CASE(2) GPK_MM_CASE(3) GPK_MM_CASE(4) GPK_MM_CASE(5) GPK_MM_CASE(6) GPK_MM_CASE(7) GPK_MM_CASE(8)
    GPK_MM_CASE(9) GPK_MM_CASE(10) GPK_MM_CASE(11) GPK_MM_CASE(12) GPK_MM_CASE(13) GPK_MM_CASE(14) GPK_MM_CASE(15) GPK_MM_CASE(16)
#undef GPK_MM_CASE
  }
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

void mm_finish(gpk_handle h, const MomK& k, const MomWork& w, const StageView& v, int R) {
  hipLaunchKernelGGL(moments_finish_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, v, R, w.G_, w.nrw, w.NV, (const double*)w.Sz,
                     (const double*)w.Bm, (const double*)w.rowpart, (const double*)w.pairpart);
}

// Every check of the model arguments (GPK_BAD_ARG before anything is launched) and the kernels' parameter block.
int mm_models(gpk_handle h, const std::string& who, const HostModels& m, bool chain, MomK& k) {
  GPK_REQUIRE(h, h->batch == 1, who + "not available in batched mode");
  GPK_REQUIRE(h, m.X && m.alpha && m.ls && m.sf2 && m.y_mean && m.y_std && m.kss, who + "null pointer");
  GPK_REQUIRE(h, m.W, who + "null K^-1 or Q (the lower tiles, as gpk_wtw writes them)");
  GPK_REQUIRE(h, m.B >= 1 && m.B <= GPK_SMALL_MAX_MODELS, who + "1..8 models");
  GPK_REQUIRE(h, m.P >= 1 && m.P <= GPK_MAX_P && m.P <= 16 && (m.B == 1 || m.P == 1), who + "P must be in [1, 16]");
  GPK_REQUIRE(h, m.D >= 1 && m.D <= GPK_PROP_MAX_D && m.nx >= 1 && m.nx <= GPK_PROP_MAX_NX && m.nx <= m.D, who + "needs 1 <= nx <= D <= 16");
  GPK_REQUIRE(h, !chain || m.nx >= m.B * m.P, who + "the state dimension nx must not be below the number of outputs");
  GPK_REQUIRE(h, m.N >= 1 && gpk_padded(m.N) <= GPK_SMALL_MAX_NP && m.Np == gpk_padded(m.N),
              who + "needs N <= 16384 and Np = gpk_padded(N)");
  GPK_REQUIRE(h, m.ldw >= m.Np, who + "needs ldk >= Np");
  GPK_REQUIRE(h, !m.var_includes_noise || m.noise, who + "null noise levels");
  GPK_REQUIRE(h, (m.in_shift == nullptr) == (m.in_scale == nullptr), who + "in_shift and in_scale go together");
  const int NO = m.B * m.P;
  for (int b = 0; b < m.B; ++b) GPK_REQUIRE(h, m.X[b] && m.alpha[b], who + "null model pointer");
  for (int b = 0; b < m.B; ++b) GPK_REQUIRE(h, m.W[b], who + "null K^-1 or Q (the lower tiles, as gpk_wtw writes them)");
  GPK_REQUIRE(h, gpk_finite(m.ls, (size_t)m.B * m.D) && gpk_finite(m.sf2, m.B) && gpk_finite(m.y_mean, NO) && gpk_finite(m.y_std, NO),
              who + "ls, sf2, y_mean and y_std must not contain NaN or infinity");
  for (int i = 0; i < m.B * m.D; ++i) GPK_REQUIRE(h, m.ls[i] > 0.0, who + "length-scales must be positive");
  for (int b = 0; b < m.B; ++b) GPK_REQUIRE(h, m.sf2[b] > 0.0, who + "sf2 must be positive");
  GPK_REQUIRE(h, gpk_finite(m.kss, m.B) && gpk_finite(&m.floor_, 1) && (!m.var_includes_noise || gpk_finite(m.noise, m.B)),
              who + "kss, floor and noise must be finite");
  k = MomK{};
  k.B = m.B; k.P = m.P; k.D = m.D; k.nx = m.nx; k.NO = NO; k.U = m.B * (m.B + 1) / 2;
  k.N = m.N; k.Np = m.Np; k.ldk = m.ldw;
  k.floor_ = m.floor_;
  k.add_noise = m.var_includes_noise != 0;
  for (int d = 0; d < 16; ++d) { k.in_shift[d] = 0.0; k.in_scale[d] = 1.0; k.model_of[d] = -1; }
  for (int b = 0; b < m.B; ++b) {
    k.X[b] = m.X[b]; k.alpha[b] = m.alpha[b]; k.Kinv[b] = m.W[b];
    for (int d = 0; d < m.D; ++d) k.ls[b][d] = m.ls[(size_t)b * m.D + d];
    k.lsf2[b] = log(m.sf2[b]);
    k.kss[b] = m.kss[b];
    k.noise[b] = m.var_includes_noise ? m.noise[b] : 0.0;
  }
  for (int o = 0; o < NO; ++o) { k.ymean[o] = m.y_mean[o]; k.ystd[o] = m.y_std[o]; }
  if (m.in_shift) {
    GPK_REQUIRE(h, gpk_finite(m.in_shift, m.D) && gpk_finite(m.in_scale, m.D), who + "the input scaler must not contain NaN or infinity");
    for (int d = 0; d < m.D; ++d) {
      GPK_REQUIRE(h, m.in_scale[d] != 0.0, who + "in_scale must be non-zero");
      k.in_shift[d] = m.in_shift[d];
      k.in_scale[d] = m.in_scale[d];
    }
    k.scaled = 1;
  }
  if (chain) {
    for (int o = 0; o < NO; ++o) {
      const int c = m.coord ? m.coord[o] : o;
      GPK_REQUIRE(h, c >= 0 && c < m.nx, who + "coord must be in [0, nx)");
      GPK_REQUIRE(h, k.model_of[c] < 0, who + "coord must be distinct");
      k.model_of[c] = o;
    }
  }
  return GPK_OK;
}

// ---- the adjoint of the moments (K11, "gradient through the moments") ---------------------------------------------------------------
// Seeds e~ (on E[mu]), V~ (symmetric, on V) and C~ (on Cov[z_x, mu]) in normalised units; results m~ (D) and S~ (nx x nx).  With B =
// (S + Lam_b)^-1 on the state block and 1 / Lam_b elsewhere, e^_o = e~_o - 2 (V~ E[mu])_o and t~_o = B S C~_o:
//   mean part, model b:   w_i = l_i sum_o alpha_io (e^_o + t~_o . nu_i,x);   W0, W1, W2 = sum_i w_i {1, nu_i, nu_i,x nu_i,x^T}
//                         m~ += B W1 - sum_o t~_o E[mu_o],   S~ += B W2 B / 2 - W0 B / 2 + sum_o (C~_o - t~_o) (B sum_i alpha_io l_i nu_i)^T
//   pair (a, b):          c_ij = alpha_i^T V~ alpha_j - kappa (K^-1)_ij, kappa = sum_p V~_pp [E[v_p] > floor]  (a batch pair: V~_ab
//                         alpha_i alpha_j, twice for a != b, kappa = V~_bb [..] on a == b);  zeta_ij = P_a nu_i + P_b nu_j
//                         A0, A1, A2 = sum_ij c_ij L_ij {1, zeta_ij, zeta_ij,x zeta_ij,x^T}:   NV = 1 + D + nx (nx + 1) / 2 sums
//                         m~_x += R^-T A1_x, m~_u += A1_u,  S~ += R^-T A2 R^-1 / 2 - A0 (S + P_ab^-1)^-1 / 2
// with R^-T = I - P_ab G G^T and (S + P_ab^-1)^-1 = R^-T P_ab from the forward setup's factor: nothing inverts S.  S~ is symmetrised
// at the end.  Launches, behind the forward's five:
//   moments_keep_kernel          E[mu] and the clip indicators [E[v] > floor] of the batch, from the forward's slots
//   moments_grad_setup_kernel    one wave per (query, model or pair): the normalised seeds, e^, t~, R^-T, kappa
//   moments_grad_row_kernel      the N rows: w_i and the workgroups' shares of W0, W1, W2;  P_b nu_i per (model, query)
//   moments_pair_grad_kernel     the forward pair kernel's tiles, masks, query loop and query groups; the exponent from the same row
//                                vectors; V~ alpha_i of the tile's rows formed in LDS per query; the NV sums through the chunked LDS
//                                reduction into the workgroup's own slot, c_ij L_ij of the thread's 4 x 4 pairs in registers throughout.
//                                No atomics.  Templated on the capacity PC >= P of its alpha tiles (1: every batch; 8; 16) - nx and
//                                D are loop bounds, the sums are indexed at run time
//   moments_grad_finish_kernel   one workgroup per query: the slots in workgroup order, m~ and S~ (lower triangle, mirrored), the raw
//                                units dq = dz / in_scale, dSigma = dS / (in_scale in_scale^T) and - in the chain - the adjoint step.
constexpr int MG_GS = 40;          // doubles per (query, output) of the setup: t~ (16), C~ - t~ (16), e^ (at 32)

struct MomSeeds {
  const double *gmean, *gcov, *gxcov;      // a query batch: raw seeds R x NO, R x NO x NO, R x NO x D on the device, null: zero
  const double *lam, *Lam, *lin;           // the chain (lam non-null): the incoming adjoints R x nx, R x nx x nx, and lin
};
// the chain's adjoint step of stage h in the finishing launch (lam null: none)
struct MomAdj {
  const double *lin, *gx_h, *gS_h;
  double *lam, *Lam, *dU;
  int H, h;
};

// grid R, 64 threads: keepE[r][16] = E[mu_o], keepF[r][U] = [E[v_b] > floor] of the diagonal pairs, the slots added as the finishing
// launch adds them
__global__ __launch_bounds__(64) void moments_keep_kernel(MomK k, int R, int G_, int nrw, int NV, const double* __restrict__ rowpart,
                                                          const double* __restrict__ pairpart, double* keepE, double* keepF) {
  const int tid = threadIdx.x, r = blockIdx.x;
  if (tid < 16) {
    double s = 0.0;
    if (tid < k.NO)
      for (int w = 0; w < nrw; ++w) s += rowpart[(((long long)w * R + r) * k.NO + tid) * MM_WS + 16];
    keepE[r * 16 + tid] = s;
  }
  if (tid < k.U) {
    int a, b;
    pair_of(tid, a, b);
    double f = 0.0;
    if (a == b) {
      const double* p = pairpart + ((long long)tid * G_ * R + r) * NV;
      double s = 0.0;
      for (int g = 0; g < G_; ++g) s += p[(long long)g * R * NV];
      f = k.kss[b] - s > k.floor_ ? 1.0 : 0.0;
    }
    keepF[r * k.U + tid] = f;
  }
}

// What the taped set-up launch reads in the place of keepE / keepF: the stage's forward slots, still in the horizon's block.
struct MomTape {
  const double *rowpart, *pairpart;
  double* keepE;                     // written by unit 0 for the finishing launch
  int G_, nrw, NV;
};

// The body of the two set-up kernels below.  TAPED: E[mu_o] and the clip indicators are formed here from the forward's slots, in
// moments_keep_kernel's order (w ascending; g ascending) - every unit of a query redoes the few sums it needs, unit 0 stores
// keepE; no atomics, no tickets, no spin.  Not TAPED: they are read from keepE / keepF, instruction for instruction as before.
template <bool TAPED>
__device__ __forceinline__ void mg_setup_body(const MomK& k, const MomSeeds& sd, int R, const double* __restrict__ Sz,
                                              const double* __restrict__ Bm, const double* __restrict__ G,
                                              const double* __restrict__ keepE, const double* __restrict__ keepF, const MomTape& tp,
                                              double* gs, double* gsV, double* RiT, double* kap) {
  __shared__ double S[16][17], Vb[16][17], Cb[16][17], T[16][17], eb[16], Em[16];
  __shared__ int cof[16];
  const int lane = threadIdx.x, r = blockIdx.x, unit = blockIdx.y, nx = k.nx, NO = k.NO, D = k.D, P = k.P;
  if (lane < 16) {
    int c = 0;
    for (int d = 0; d < nx; ++d)
      if (k.model_of[d] == lane) c = d;
    cof[lane] = c;
  }
  for (int e = lane; e < 256; e += 64) S[e >> 4][e & 15] = Sz[(long long)r * 256 + e];
  __syncthreads();
  for (int e = lane; e < 256; e += 64) {
    const int i = e >> 4, j = e & 15;
    double v = 0.0, c = 0.0;
    if (i < NO && j < NO) {
      double g = 0.0;
      if (sd.lam) g = sd.Lam[((long long)r * nx + cof[i]) * nx + cof[j]];
      else if (sd.gcov) g = 0.5 * (sd.gcov[((long long)r * NO + i) * NO + j] + sd.gcov[((long long)r * NO + j) * NO + i]);
      v = g * (k.ystd[i] * k.ystd[j]);
    }
    if (i < NO && j < nx) {
      double g = 0.0;
      if (sd.lam) {      // 2 (E^T Lam A0)(o, j)
        for (int c2 = 0; c2 < nx; ++c2)
          g = __builtin_fma(sd.Lam[((long long)r * nx + cof[i]) * nx + c2], (c2 == j ? 1.0 : 0.0) + sd.lin[c2 * D + j], g);
        g *= 2.0;
      } else if (sd.gxcov) {
        g = sd.gxcov[((long long)r * NO + i) * D + j];
      }
      c = g * k.ystd[i] * (k.scaled ? k.in_scale[j] : 1.0);
    }
    Vb[i][j] = v;
    Cb[i][j] = c;
  }
  if (lane < 16) {
    double g = 0.0;
    if (lane < NO) g = sd.lam ? sd.lam[(long long)r * nx + cof[lane]] : sd.gmean ? sd.gmean[(long long)r * NO + lane] : 0.0;
    eb[lane] = lane < NO ? g * k.ystd[lane] : 0.0;
    if constexpr (TAPED) {
      double s = 0.0;
      if (lane < NO)
        for (int w = 0; w < tp.nrw; ++w) s += tp.rowpart[(((long long)w * R + r) * NO + lane) * MM_WS + 16];
      Em[lane] = s;
      if (unit == 0) tp.keepE[r * 16 + lane] = s;
    } else {
      Em[lane] = keepE[r * 16 + lane];
    }
  }
  __syncthreads();
  if (unit < k.B) {
    if (unit == 0)
      for (int e = lane; e < 256; e += 64) gsV[(long long)r * 256 + e] = Vb[e >> 4][e & 15];
    // T[p] = S C~_o, then t~_o = Bm T[p]
    const double* bm = Bm + ((long long)r * k.B + unit) * 256;
    for (int e = lane; e < P * 16; e += 64) {
      const int p = e >> 4, i = e & 15, o = unit * P + p;
      double s = 0.0;
      for (int c = 0; c < nx; ++c) s = __builtin_fma(S[i][c], Cb[o][c], s);
      T[p][i] = s;
    }
    __syncthreads();
    for (int e = lane; e < P * 16; e += 64) {
      const int p = e >> 4, i = e & 15, o = unit * P + p;
      double s = 0.0;
      if (i < nx)
        for (int c = 0; c < nx; ++c) s = __builtin_fma(bm[i * 16 + c], T[p][c], s);
      double* o_ = gs + ((long long)r * NO + o) * MG_GS;
      o_[i] = s;
      o_[16 + i] = i < nx ? Cb[o][i] - s : 0.0;
      if (i == 0) {
        double v = 0.0;
        for (int c = 0; c < NO; ++c) v = __builtin_fma(Vb[o][c], Em[c], v);
        o_[32] = eb[o] - 2.0 * v;
      }
    }
    return;
  }
  const int u = unit - k.B;
  int a, b;
  pair_of(u, a, b);
  const double* g = G + ((long long)r * k.U + u) * 256;
  for (int e = lane; e < 256; e += 64) T[e >> 4][e & 15] = g[e];
  __syncthreads();
  for (int e = lane; e < 256; e += 64) {
    const int i = e >> 4, j = e & 15;
    double v = 0.0;
    if (i < nx && j < nx) {
      double m = 0.0;
      for (int c = 0; c < nx; ++c) m = __builtin_fma(T[i][c], T[j][c], m);
      const double la = k.ls[a][i], lb = k.ls[b][i];
      v = (i == j ? 1.0 : 0.0) - (1.0 / (la * la) + 1.0 / (lb * lb)) * m;
    }
    RiT[((long long)r * k.U + u) * 256 + e] = v;
  }
  double clip = 0.0;      // [E[v_b] > floor] of a diagonal pair (lane 0)
  if constexpr (TAPED) {
    // the pair's G_ <= MM_MAXG slots of the K^-1 sum: loaded side by side, added by lane 0 in workgroup order
    __shared__ double pg[MM_MAXG];
    if (a == b) {
      const double* p = tp.pairpart + ((long long)u * tp.G_ * R + r) * tp.NV;
      for (int g2 = lane; g2 < tp.G_; g2 += 64) pg[g2] = p[(long long)g2 * R * tp.NV];
    }
    __syncthreads();
    if (lane == 0 && a == b) {
      double s = 0.0;
      for (int g2 = 0; g2 < tp.G_; ++g2) s += pg[g2];
      clip = k.kss[b] - s > k.floor_ ? 1.0 : 0.0;
    }
  } else if (lane == 0 && a == b) {
    clip = keepF[r * k.U + u];
  }
  if (lane == 0) {
    double v = 0.0;
    if (a == b) {
      if (k.B > 1) v = Vb[a][a];
      else
        for (int p = 0; p < P; ++p) v += Vb[p][p];
      v *= clip;
    }
    kap[r * k.U + u] = v;
  }
}

// grid (R, B + U), 64 threads.  Units [0, B): gs[(r NO + o) MG_GS ..] of the model's outputs; unit 0 also gsV[r][16][16] = V~.
// Units [B, B + U): RiT[(r U + u) 256 ..] = R^-T (zero beyond nx) and kap[r U + u].
__global__ __launch_bounds__(64) void moments_grad_setup_kernel(MomK k, MomSeeds sd, int R, const double* __restrict__ Sz,
                                                                const double* __restrict__ Bm, const double* __restrict__ G,
                                                                const double* __restrict__ keepE, const double* __restrict__ keepF,
                                                                double* gs, double* gsV, double* RiT, double* kap) {
  mg_setup_body<false>(k, sd, R, Sz, Bm, G, keepE, keepF, MomTape{}, gs, gsV, RiT, kap);
}

// The same on a taped stage (gpk_mm_chain_grad with the tape): the keep launch's sums made here, so that the backward sweep of a
// stage is four launches.  Same grid.
__global__ __launch_bounds__(64) void moments_grad_setup_taped_kernel(MomK k, MomSeeds sd, int R, MomTape tp,
                                                                      const double* __restrict__ Sz, const double* __restrict__ Bm,
                                                                      const double* __restrict__ G, double* gs, double* gsV,
                                                                      double* RiT, double* kap) {
  mg_setup_body<true>(k, sd, R, Sz, Bm, G, nullptr, nullptr, tp, gs, gsV, RiT, kap);
}

// grid (ceil(N / 256), R, B), 256 threads.  part[((wg R + r) B + b) NV + v]: the workgroup's shares of W0 (v = 0), W1 (1 + d) and
// W2 (1 + D + c (c + 1) / 2 + d, d <= c < nx), the rows added in row order;  gp[((b R + r) Np + i) 16 + d] = (P_b nu_i)_d.
__global__ __launch_bounds__(256) void moments_grad_row_kernel(MomK k, int NV, const double* __restrict__ q, const double* __restrict__ Bm,
                                                               const double* __restrict__ cm, const double* __restrict__ gs, double* gp,
                                                               double* part) {
  __shared__ double sB[16][17], nuS[MM_ROWS][MM_WS], z[16], ip[16], tb[16][17], eh[16];
  const int tid = threadIdx.x, r = blockIdx.y, b = blockIdx.z, R = gridDim.y, D = k.D, nx = k.nx, P = k.P;
  const long long row = (long long)blockIdx.x * MM_ROWS + tid;
  sB[tid >> 4][tid & 15] = Bm[((long long)r * k.B + b) * 256 + tid];
  if (tid < 16) {
    z[tid] = tid < D ? q[(long long)r * D + tid] : 0.0;
    ip[tid] = tid < D ? 1.0 / (k.ls[b][tid] * k.ls[b][tid]) : 0.0;
    eh[tid] = tid < P ? gs[((long long)r * k.NO + b * P + tid) * MG_GS + 32] : 0.0;
  }
  {
    const int p = tid >> 4, d = tid & 15;
    tb[p][d] = p < P ? gs[((long long)r * k.NO + b * P + p) * MG_GS + d] : 0.0;
  }
  __syncthreads();
  const bool live = row < k.N;
  const double* xr = k.X[b] + row * D;
  double nu[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) nu[d] = (live && d < D) ? xr[d] - z[d] : 0.0;
  double quad = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i < nx) {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) t = __builtin_fma(sB[i][j], nu[j], t);
      quad = __builtin_fma(nu[i], t, quad);
    } else {
      quad = __builtin_fma(nu[i] * nu[i], ip[i], quad);
    }
  }
  const double l = live ? exp(cm[(long long)r * k.B + b] - 0.5 * quad) : 0.0;
  double w = 0.0;
  for (int p = 0; p < P; ++p) {
    double dot = eh[p];
#pragma unroll
    for (int d = 0; d < 16; ++d) dot = __builtin_fma(tb[p][d], nu[d], dot);      // (entries >= nx of t~ are zero)
    const double al = live ? k.alpha[b][row * P + p] : 0.0;
    w = __builtin_fma(al, dot, w);
  }
#pragma unroll
  for (int d = 0; d < 16; ++d) nuS[tid][d] = nu[d];
  nuS[tid][16] = w * l;
  if (live) {
    double* o = gp + (((long long)b * R + r) * k.Np + row) * 16;
#pragma unroll
    for (int d = 0; d < 16; ++d) o[d] = nu[d] * ip[d];
  }
  __syncthreads();
  if (tid < NV) {
    int c = 16, d = 16;      // (16: the factor is one)
    if (tid >= 1 + D) {
      const int e = tid - 1 - D;
      c = 0;
      while ((c + 1) * (c + 2) / 2 <= e) ++c;
      d = e - c * (c + 1) / 2;
    } else if (tid >= 1) {
      c = tid - 1;
    }
    double s = 0.0;
    for (int t = 0; t < MM_ROWS; ++t) {
      double f = nuS[t][16];
      if (c < 16) f *= nuS[t][c];
      if (d < 16) f *= nuS[t][d];
      s += f;
    }
    part[((((long long)blockIdx.x * R + r) * k.B + b)) * NV + tid] = s;
  }
}

// grid (G, U, NQ), 256 threads, thread (ty, tx) as in moments_pair_kernel.  part[((u G + g) R + r) NV + v]: v = 0 A0, 1 + d A1,
// 1 + D + c (c + 1) / 2 + d A2 (d <= c < nx).  An off-diagonal tile of a == b stands for its mirror image too: c_ij, L_ij and
// zeta_ij are symmetric in (i, j) there, so its sums count twice.
template <int PC, bool SPLIT>
__global__ __launch_bounds__(256) void moments_pair_grad_kernel(MomK k, int R, int NV, const double* __restrict__ rowq,
                                                                const double* __restrict__ cl, const double* __restrict__ gp,
                                                                const double* __restrict__ gsV, const double* __restrict__ kap,
                                                                double* part) {
  __shared__ double sA[MM_TILE][PC], sB[MM_TILE][PC], sVa[MM_TILE][PC], sV[PC][PC], sWa[MM_TILE][MM_WS], sWb[MM_TILE][MM_WS],
      sPa[MM_TILE][MM_WS], sPb[MM_TILE][MM_WS], red[MM_CH][16 * 17], red2[MM_CH][16];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, u = blockIdx.y, g = blockIdx.x, G_ = gridDim.x, nx = k.nx, D = k.D, P = k.P;
  const int r0 = SPLIT ? (int)(blockIdx.z * (unsigned)R / gridDim.z) : 0;
  const int r1 = SPLIT ? (int)((blockIdx.z + 1) * (unsigned)R / gridDim.z) : R;
  int a, b;
  pair_of(u, a, b);
  const bool same = a == b;
  const long long N = k.N;
  const int nt = (int)((N + MM_TILE - 1) / MM_TILE);
  const long long ntiles = same ? (long long)nt * (nt + 1) / 2 : (long long)nt * nt;
  const double* Wa = rowq + (long long)(a * a + 2 * b) * R * k.Np * MM_WS;
  const double* Wb = same ? Wa : Wa + (long long)R * k.Np * MM_WS;
  const double* Pa = gp + (long long)a * R * k.Np * 16;
  const double* Pb = gp + (long long)b * R * k.Np * 16;
  bool first = true;
  for (long long t = g; t < ntiles; t += G_) {
    int ti, tj;
    if (same) {
      ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
      while ((long long)(ti + 1) * (ti + 2) / 2 <= t) ++ti;
      while ((long long)ti * (ti + 1) / 2 > t) --ti;
      tj = (int)(t - (long long)ti * (ti + 1) / 2);
    } else {
      ti = (int)(t / nt);
      tj = (int)(t % nt);
    }
    const double wgt = (same && ti != tj) ? 2.0 : 1.0;
    const long long i0 = (long long)ti * MM_TILE, j0 = (long long)tj * MM_TILE;
    double kv[4][4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const long long i = i0 + ty + 16 * ii, j = j0 + tx + 16 * jj;
        kv[ii][jj] = (same && i < N && j < N) ? k.Kinv[a][(i > j ? i : j) * k.ldk + (i > j ? j : i)] : 0.0;
      }
    __syncthreads();
    for (int e = tid; e < MM_TILE * P; e += 256) {
      const int row = e / P, p = e % P;
      sA[row][p] = i0 + row < N ? k.alpha[a][(i0 + row) * P + p] : 0.0;
      sB[row][p] = j0 + row < N ? k.alpha[b][(j0 + row) * P + p] : 0.0;
    }
    for (int r = r0; r < r1; ++r) {
      __syncthreads();
      for (int e = tid; e < MM_TILE * MM_WS; e += 256) {
        const int row = e / MM_WS;
        sWa[row][e % MM_WS] = i0 + row < N ? Wa[((long long)r * k.Np + i0) * MM_WS + e] : 0.0;
        sWb[row][e % MM_WS] = j0 + row < N ? Wb[((long long)r * k.Np + j0) * MM_WS + e] : 0.0;
      }
      for (int e = tid; e < MM_TILE * 16; e += 256) {
        const int row = e >> 4;
        sPa[row][e & 15] = i0 + row < N ? Pa[((long long)r * k.Np + i0) * 16 + e] : 0.0;
        sPb[row][e & 15] = j0 + row < N ? Pb[((long long)r * k.Np + j0) * 16 + e] : 0.0;
      }
      // V~ of the pair: the P x P block of one model, or the batch pair's entry (both orders of a != b)
      if (tid < P * P)
        sV[tid / P][tid % P] = k.B > 1 ? (same ? 1.0 : 2.0) * gsV[(long long)r * 256 + a * 16 + b]
                                       : gsV[(long long)r * 256 + (tid / P) * 16 + tid % P];
      __syncthreads();
      for (int e = tid; e < MM_TILE * P; e += 256) {
        const int row = e / P, p = e % P;
        double s = 0.0;
        for (int c = 0; c < P; ++c) s = __builtin_fma(sV[p][c], sA[row][c], s);
        sVa[row][p] = s;
      }
      const double c0 = cl[(long long)r * k.U + u];
      double ex[4][4];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) ex[ii][jj] = (c0 + sWa[ty + 16 * ii][16]) + sWb[tx + 16 * jj][16];
      for (int c = 0; c < nx; ++c) {
        double wa[4], wb[4];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) { wa[ii] = sWa[ty + 16 * ii][c]; wb[ii] = sWb[tx + 16 * ii][c]; }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) ex[ii][jj] = __builtin_fma(wa[ii], wb[jj], ex[ii][jj]);
      }
      __syncthreads();
      // e_ij = c_ij L_ij of the thread's pairs, kept to the end of the tile's sums
      const double kp = kap[(long long)r * k.U + u];
      double cw[4][4];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) cw[ii][jj] = -kp * kv[ii][jj];
      for (int p = 0; p < P; ++p) {
        double va[4], bj[4];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) { va[ii] = sVa[ty + 16 * ii][p]; bj[ii] = sB[tx + 16 * ii][p]; }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) cw[ii][jj] = __builtin_fma(va[ii], bj[jj], cw[ii][jj]);
      }
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const bool live = i0 + ty + 16 * ii < N && j0 + tx + 16 * jj < N;
          ex[ii][jj] = live ? cw[ii][jj] * exp(ex[ii][jj]) : 0.0;
        }
      double er[4], ec[4];      // the block's row and column sums of e
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        er[ii] = (ex[ii][0] + ex[ii][1]) + (ex[ii][2] + ex[ii][3]);
        ec[ii] = (ex[0][ii] + ex[1][ii]) + (ex[2][ii] + ex[3][ii]);
      }
      double* slot = part + (((long long)u * G_ + g) * R + r) * NV;
      auto flush = [&](int chunk, int nvals) {
        __syncthreads();
        if (ty < nvals) {
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < 16; ++c) s += red[ty][tx * 17 + c];
          red2[ty][tx] = s;
        }
        __syncthreads();
        if (tid < nvals) {
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < 16; ++c) s += red2[tid][c];
          s *= wgt;
          double* dst = slot + chunk * MM_CH + tid;
          *dst = first ? s : *dst + s;
        }
      };
      auto emit = [&](int v, double x) {
        red[v % MM_CH][ty * 17 + tx] = x;
        if (v % MM_CH == MM_CH - 1 || v == NV - 1) flush(v / MM_CH, v % MM_CH + 1);
      };
      emit(0, (er[0] + er[1]) + (er[2] + er[3]));
      for (int d = 0; d < D; ++d) {      // A1_d = sum_i p^a_id er_i + sum_j p^b_jd ec_j
        double s = 0.0;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) s = __builtin_fma(sPa[ty + 16 * ii][d], er[ii], s);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) s = __builtin_fma(sPb[tx + 16 * jj][d], ec[jj], s);
        emit(1 + d, s);
      }
      int v = 1 + D;
      for (int c = 0; c < nx; ++c) {
        // ga_i = sum_j e_ij (p^a_ic + p^b_jc), gb_j = sum_i e_ij (p^a_ic + p^b_jc):  A2_cd = sum_i p^a_id ga_i + sum_j p^b_jd gb_j
        double pa[4], pb[4], ga[4], gb[4];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) { pa[ii] = sPa[ty + 16 * ii][c]; pb[ii] = sPb[tx + 16 * ii][c]; }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) { ga[ii] = er[ii] * pa[ii]; gb[ii] = ec[ii] * pb[ii]; }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            ga[ii] = __builtin_fma(ex[ii][jj], pb[jj], ga[ii]);
            gb[jj] = __builtin_fma(ex[ii][jj], pa[ii], gb[jj]);
          }
        for (int d = 0; d <= c; ++d) {
          double s = 0.0;
#pragma unroll
          for (int ii = 0; ii < 4; ++ii) s = __builtin_fma(sPa[ty + 16 * ii][d], ga[ii], s);
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) s = __builtin_fma(sPb[tx + 16 * jj][d], gb[jj], s);
          emit(v++, s);
        }
      }
    }
    first = false;
  }
}

// grid R, 256 threads, thread (i, j) = (tid >> 4, tid & 15).  dq (R x D) and dS (R x nx x nx) in raw units, null where not wanted;
// with ad.lam the adjoint step of the chain's stage:  g_q = [I 0]^T lam + lin^T lam + dq,  lam <- gx_h + g_q[:nx],  dU_h = g_q[nx:],
// Lam <- gS_h + A0^T Lam A0 + dS (lower triangle formed and mirrored).
__global__ __launch_bounds__(256) void moments_grad_finish_kernel(MomK k, MomAdj ad, int R, int G_, int nrw, int NV,
                                                                  const double* __restrict__ Bm, const double* __restrict__ rowpart,
                                                                  const double* __restrict__ keepE, const double* __restrict__ gs,
                                                                  const double* __restrict__ RiT, const double* __restrict__ growpart,
                                                                  const double* __restrict__ gpairpart, double* dq, double* dS) {
  __shared__ double sv[160], Mt[16][17], W2[16][17], T1[16][17], Cz[16][17], Tm[16][17], Sb[16][17], Sr[16][17], mr[16], lm[16];
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, r = blockIdx.x;
  const int nx = k.nx, D = k.D, NO = k.NO, P = k.P, B = k.B;
  double sacc = 0.0, macc = 0.0;      // S~(i, j) before the symmetrisation; m~(tid), tid < D
  for (int b = 0; b < B; ++b) {
    if (tid < NV) {
      double s = 0.0;
      for (int w = 0; w < nrw; ++w) s += growpart[(((long long)w * R + r) * B + b) * NV + tid];
      sv[tid] = s;
    }
    Mt[i][j] = Bm[((long long)r * B + b) * 256 + tid];
    if (i < P && j < nx) {
      double s = 0.0;
      for (int w = 0; w < nrw; ++w) s += rowpart[(((long long)w * R + r) * NO + b * P + i) * MM_WS + j];
      Cz[i][j] = s;
    }
    __syncthreads();
    if (i < nx && j < nx) W2[i][j] = sv[1 + D + (i > j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i)];
    if (i < P && j < nx) {
      double s = 0.0;
      for (int c = 0; c < nx; ++c) s = __builtin_fma(Mt[j][c], Cz[i][c], s);
      Tm[i][j] = s;
    }
    __syncthreads();
    if (i < nx && j < nx) {
      double s = 0.0;
      for (int c = 0; c < nx; ++c) s = __builtin_fma(Mt[i][c], W2[c][j], s);
      T1[i][j] = s;
    }
    __syncthreads();
    if (i < nx && j < nx) {
      double s = 0.0;
      for (int c = 0; c < nx; ++c) s = __builtin_fma(T1[i][c], Mt[c][j], s);
      s = 0.5 * s - 0.5 * sv[0] * Mt[i][j];
      for (int p = 0; p < P; ++p) s = __builtin_fma(gs[((long long)r * NO + b * P + p) * MG_GS + 16 + i], Tm[p][j], s);
      sacc += s;
    }
    if (tid < D) {
      double s = 0.0;
      if (tid < nx) {
        for (int c = 0; c < nx; ++c) s = __builtin_fma(Mt[tid][c], sv[1 + c], s);
        for (int p = 0; p < P; ++p) s -= gs[((long long)r * NO + b * P + p) * MG_GS + tid] * keepE[r * 16 + b * P + p];
      } else {
        s = sv[1 + tid] / (k.ls[b][tid] * k.ls[b][tid]);
      }
      macc += s;
    }
    __syncthreads();
  }
  for (int u = 0; u < k.U; ++u) {
    int a, b;
    pair_of(u, a, b);
    if (tid < NV) {
      const double* p = gpairpart + ((long long)u * G_ * R + r) * NV + tid;
      double s = 0.0;
#pragma unroll 8
      for (int g = 0; g < G_; ++g) s += p[(long long)g * R * NV];
      sv[tid] = s;
    }
    Mt[i][j] = RiT[((long long)r * k.U + u) * 256 + tid];
    __syncthreads();
    if (i < nx && j < nx) W2[i][j] = sv[1 + D + (i > j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i)];
    __syncthreads();
    if (i < nx && j < nx) {
      double s = 0.0;
      for (int c = 0; c < nx; ++c) s = __builtin_fma(Mt[i][c], W2[c][j], s);
      T1[i][j] = s;
    }
    __syncthreads();
    if (i < nx && j < nx) {
      double s = 0.0;
      for (int c = 0; c < nx; ++c) s = __builtin_fma(T1[i][c], Mt[j][c], s);
      const double la = k.ls[a][j], lb = k.ls[b][j];
      sacc += 0.5 * s - 0.5 * sv[0] * (Mt[i][j] * (1.0 / (la * la) + 1.0 / (lb * lb)));
    }
    if (tid < D) {
      double s = 0.0;
      if (tid < nx)
        for (int c = 0; c < nx; ++c) s = __builtin_fma(Mt[tid][c], sv[1 + c], s);
      else
        s = sv[1 + tid];
      macc += s;
    }
    __syncthreads();
  }
  Sb[i][j] = (i < nx && j < nx) ? sacc : 0.0;
  if (tid < 16) mr[tid] = tid < D ? (k.scaled ? macc / k.in_scale[tid] : macc) : 0.0;
  __syncthreads();
  if (i < nx && j <= i) {
    double s = 0.5 * (Sb[i][j] + Sb[j][i]);
    if (k.scaled) s = s / (k.in_scale[i] * k.in_scale[j]);
    Sr[i][j] = s;
    Sr[j][i] = s;
  }
  __syncthreads();
  if (dq && tid < D) dq[(long long)r * D + tid] = mr[tid];
  if (dS && i < nx && j < nx) dS[((long long)r * nx + i) * nx + j] = Sr[i][j];
  if (!ad.lam) return;
  // the adjoint step: Mt = Lam, W2 = A0
  if (i < nx && j < nx) {
    Mt[i][j] = ad.Lam[((long long)r * nx + i) * nx + j];
    W2[i][j] = (i == j ? 1.0 : 0.0) + ad.lin[i * D + j];
  }
  if (tid < nx) lm[tid] = ad.lam[(long long)r * nx + tid];
  __syncthreads();
  if (tid < D) {
    double s = tid < nx ? lm[tid] : 0.0;
    for (int c = 0; c < nx; ++c) s = __builtin_fma(ad.lin[c * D + tid], lm[c], s);
    s += mr[tid];
    if (tid < nx) ad.lam[(long long)r * nx + tid] = ad.gx_h[(long long)r * nx + tid] + s;
    else ad.dU[((long long)r * ad.H + ad.h) * (D - nx) + (tid - nx)] = s;
  }
  if (i < nx && j < nx) {
    double t = 0.0;
    for (int c = 0; c < nx; ++c) t = __builtin_fma(Mt[i][c], W2[c][j], t);
    T1[i][j] = t;
  }
  __syncthreads();
  if (i < nx && j <= i) {
    double s = 0.0;
    for (int c = 0; c < nx; ++c) s = __builtin_fma(W2[c][i], T1[c][j], s);
    const long long at = (long long)r * nx * nx;
    if (ad.gS_h) s += ad.gS_h[at + i * nx + j];
    s += Sr[i][j];
    ad.Lam[at + i * nx + j] = s;
    ad.Lam[at + j * nx + i] = s;
  }
}

// The adjoint's device work area for one batch of R queries, behind the forward's (MomWork), carved from `base`.
struct MomGradWork {
  double *keepE, *keepF, *gs, *gsV, *RiT, *kap, *gp, *rowpart, *pairpart;
  int NV;
  size_t doubles;
};

MomGradWork mg_work(const MomK& k, const MomWork& w, int R, double* base) {
  MomGradWork g{};
  g.NV = 1 + k.D + k.nx * (k.nx + 1) / 2;
  size_t at = 0;
  auto take = [&](size_t n) { double* p = base ? base + at : nullptr; at += n; return p; };
  g.keepE = take((size_t)R * 16);
  g.keepF = take((size_t)R * k.U);
  g.gs = take((size_t)R * k.NO * MG_GS);
  g.gsV = take((size_t)R * 256);
  g.RiT = take((size_t)R * k.U * 256);
  g.kap = take((size_t)R * k.U);
  g.gp = take((size_t)k.B * R * k.Np * 16);
  g.rowpart = take((size_t)w.nrw * R * k.B * g.NV);
  g.pairpart = take((size_t)k.U * w.G_ * R * g.NV);
  g.doubles = at;
  return g;
}

void mm_keep(gpk_handle h, const MomK& k, const MomWork& w, int R, double* keepE, double* keepF) {
  hipLaunchKernelGGL(moments_keep_kernel, dim3((unsigned)R), dim3(64), 0, h->stream, k, R, w.G_, w.nrw, w.NV, (const double*)w.rowpart,
                     (const double*)w.pairpart, keepE, keepF);
}

template <int PC>
void mg_pair_launch(gpk_handle h, const MomK& k, const MomWork& w, const MomGradWork& g, int R) {
  if (w.NQ > 1)
    hipLaunchKernelGGL((moments_pair_grad_kernel<PC, true>), dim3((unsigned)w.G_, (unsigned)k.U, (unsigned)w.NQ), dim3(256), 0,
                       h->stream, k, R, g.NV, (const double*)w.rowq, (const double*)w.cl, (const double*)g.gp, (const double*)g.gsV,
                       (const double*)g.kap, g.pairpart);
  else
    hipLaunchKernelGGL((moments_pair_grad_kernel<PC, false>), dim3((unsigned)w.G_, (unsigned)k.U), dim3(256), 0, h->stream, k, R, g.NV,
                       (const double*)w.rowq, (const double*)w.cl, (const double*)g.gp, (const double*)g.gsV, (const double*)g.kap,
                       g.pairpart);
}

// The four launches of the adjoint on a batch whose forward setup and row vectors are in w (Sz, Bm, cm, G, cl, rowq, rowpart) and
// whose E[mu] and clip indicators are in keepE / keepF: d_q the scaled queries.  taped: w also holds the forward's slots
// (rowpart, pairpart) and no keep launch has run - the set-up launch forms keepE (stored) and the indicators from them.
int mg_launch(gpk_handle h, const MomK& k, const MomWork& w, const MomGradWork& g, int R, const double* d_q, const MomSeeds& sd,
              const MomAdj& ad, double* keepE, const double* keepF, double* dq, double* dS, bool taped = false) {
  const int PC = k.P == 1 ? 1 : k.P <= 8 ? 8 : 16;      // the capacity of the pair kernel's alpha tiles: what is logged is what is launched
  if (h->gram_log)
    fprintf(stderr, "GPKMM adj %d %d %d %d %lld %d cus%d g%d u%d nq%d split%d nrw%d nv%d pc%d\n", k.B, k.P, k.D, k.nx, k.N, R, gpk_cus(h),
            w.G_, k.U, w.NQ, w.NQ > 1 ? 1 : 0, w.nrw, g.NV, PC);
  if (taped)
    hipLaunchKernelGGL(moments_grad_setup_taped_kernel, dim3((unsigned)R, (unsigned)(k.B + k.U)), dim3(64), 0, h->stream, k, sd, R,
                       MomTape{w.rowpart, w.pairpart, keepE, w.G_, w.nrw, w.NV}, (const double*)w.Sz, (const double*)w.Bm,
                       (const double*)w.G, g.gs, g.gsV, g.RiT, g.kap);
  else
    hipLaunchKernelGGL(moments_grad_setup_kernel, dim3((unsigned)R, (unsigned)(k.B + k.U)), dim3(64), 0, h->stream, k, sd, R,
                       (const double*)w.Sz, (const double*)w.Bm, (const double*)w.G, (const double*)keepE, keepF, g.gs, g.gsV, g.RiT,
                       g.kap);
  GPK_LAUNCH_CHECK(h);
  hipLaunchKernelGGL(moments_grad_row_kernel, dim3((unsigned)w.nrw, (unsigned)R, (unsigned)k.B), dim3(256), 0, h->stream, k, g.NV, d_q,
                     (const double*)w.Bm, (const double*)w.cm, (const double*)g.gs, g.gp, g.rowpart);
  GPK_LAUNCH_CHECK(h);
  if (PC == 1) mg_pair_launch<1>(h, k, w, g, R);
  else if (PC == 8) mg_pair_launch<8>(h, k, w, g, R);
  else mg_pair_launch<16>(h, k, w, g, R);
  GPK_LAUNCH_CHECK(h);
  hipLaunchKernelGGL(moments_grad_finish_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, ad, R, w.G_, w.nrw, g.NV,
                     (const double*)w.Bm, (const double*)w.rowpart, (const double*)keepE, (const double*)g.gs, (const double*)g.RiT,
                     (const double*)g.rowpart, (const double*)g.pairpart, dq, dS);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

// The forward's setup and row launches alone (the chain's backward sweep recomputes a stage's factors and row vectors with them)
int mm_launch_rows(gpk_handle h, const MomK& k, const MomWork& w, int R, const double* d_q, const double* d_S) {
  hipLaunchKernelGGL(moments_setup_kernel, dim3((unsigned)R, (unsigned)(k.B + k.U)), dim3(64), 0, h->stream, k, d_S, w.Sz, w.Bm, w.cm,
                     w.G, w.cl);
  GPK_LAUNCH_CHECK(h);
  hipLaunchKernelGGL(moments_row_mean_kernel, dim3((unsigned)w.nrw, (unsigned)R, (unsigned)k.B), dim3(256), 0, h->stream, k, d_q,
                     (const double*)w.Bm, (const double*)w.cm, w.rowpart);
  hipLaunchKernelGGL(moments_row_pair_kernel, dim3((unsigned)w.nrw, (unsigned)R, (unsigned)(2 * k.U)), dim3(256), 0, h->stream, k, d_q,
                     (const double*)w.G, w.rowq);
  GPK_LAUNCH_CHECK(h);
  return GPK_OK;
}

}  // namespace

// M <= 32 Gaussian queries: one upload [z | S], five launches, three downloads, one synchronisation.
int gpk_mm_query(gpk_handle h, const std::string& who, const HostModels& m, const double* Xq, const double* Sq, int M, double* mean,
                 double* cov, double* xcov) {
  if (!h) return GPK_BAD_ARG;
  MomK k;
  GPK_TRY(mm_models(h, who, m, false, k));
  GPK_REQUIRE(h, M >= 1 && M <= GPK_SMALL_MAX_M, who + "M must be in [1, 32]");
  GPK_REQUIRE(h, Xq && mean && cov && xcov, who + "null pointer");
  const int D = k.D, nx = k.nx, NO = k.NO;
  const size_t n_q = (size_t)M * D, n_s = (size_t)M * nx * nx;
  GPK_REQUIRE(h, gpk_finite(Xq, n_q), who + "the queries must not contain NaN or infinity");
  GPK_REQUIRE(h, !Sq || gpk_finite(Sq, n_s), who + "the covariances must not contain NaN or infinity");
  const size_t n_om = (size_t)M * NO, n_oc = n_om * NO, n_ox = n_om * D;
  const MomWork sizes = mm_work(h, k, M, nullptr);
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, (n_q + n_s + n_om + n_oc + n_ox + sizes.doubles) * sizeof(double), &ws));
  double* d_q = (double*)ws;
  double* d_S = d_q + n_q;
  double* d_om = d_S + n_s;
  double* d_oc = d_om + n_om;
  double* d_ox = d_oc + n_oc;
  const MomWork w = mm_work(h, k, M, d_ox + n_ox);
  std::vector<double> host(n_q + n_s, 0.0);
  for (int r = 0; r < M; ++r) {
    for (int d = 0; d < D; ++d) {
      const double raw = Xq[(size_t)r * D + d];
      host[(size_t)r * D + d] = k.scaled ? (raw - k.in_shift[d]) / k.in_scale[d] : raw;
    }
    if (Sq)      // the lower triangle is the matrix
      for (int i = 0; i < nx; ++i)
        for (int j = 0; j <= i; ++j)
          host[n_q + ((size_t)r * nx + i) * nx + j] = host[n_q + ((size_t)r * nx + j) * nx + i] = Sq[((size_t)r * nx + i) * nx + j];
  }
  GPK_CHECK_HIP(h, hipMemcpyAsync(d_q, host.data(), sizeof(double) * (n_q + n_s), hipMemcpyHostToDevice, h->stream));
  GPK_TRY(mm_launch(h, k, w, M, d_q, d_S));
  StageView v{};
  v.out[0] = d_om; v.out[1] = d_oc; v.out[2] = d_ox;
  mm_finish(h, k, w, v, M);
  GPK_LAUNCH_CHECK(h);
  GPK_CHECK_HIP(h, hipMemcpyAsync(mean, d_om, sizeof(double) * n_om, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(cov, d_oc, sizeof(double) * n_oc, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(xcov, d_ox, sizeof(double) * n_ox, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  return GPK_OK;
}

// The horizon chain on the skeleton of gpk_propagate.hip: one upload (the head), 5 H launches - the finishing one composes the
// stage and is what GPK_TIMED_PROPAGATE brackets - up to five downloads, one synchronisation.
int gpk_mm_chain(gpk_handle h, const std::string& who, const HostModels& m, const Horizon& z) {
  if (!h) return GPK_BAD_ARG;
  MomK k;
  GPK_TRY(mm_models(h, who, m, true, k));
  GPK_TRY(gpk_horizon_check(h, who, k.nx, k.D, z));
  const int R = z.R;
  const size_t n_om = (size_t)R * k.NO;
  HorizonBlock b(k.nx, k.D, z);
  MomWork w{};
  GPK_TRY(gpk_horizon_carve(h, b, [&] {
    b.head();
    b.outputs(n_om, z.mean, n_om * k.NO, z.cov, n_om * k.D, z.xcov);
    w = mm_work(h, k, R, b.base ? b.base + b.at : nullptr);
    b.take(w.doubles);
  }));
  std::vector<double> host(b.n_head(), 0.0);
  gpk_horizon_pack(b, z, k.scaled, k.in_shift, k.in_scale, host.data());
  GPK_TRY(gpk_horizon_upload(h, b, z, host));
  for (int s = 0; s < z.H; ++s) {
    GPK_TRY(mm_launch(h, k, w, R, b.q, b.S));
    gpk_time_begin(h, GPK_TIMED_PROPAGATE);
    mm_finish(h, k, w, gpk_horizon_stage(b, z, s), R);
    gpk_time_end(h);
    GPK_LAUNCH_CHECK(h);
  }
  return gpk_horizon_finish(h, b, z, {});
}

// gpk_mm_query with the adjoint: one upload [z | S | gmean | gcov | gxcov], the forward's five launches (mean, cov, xcov keep their
// bits), the keep launch and the adjoint's four, five downloads, one synchronisation.
int gpk_mm_query_vjp(gpk_handle h, const std::string& who, const HostModels& m, const double* Xq, const double* Sq, int M, double* mean,
                     double* cov, double* xcov, const double* gmean, const double* gcov, const double* gxcov, double* dXq, double* dSq) {
  if (!h) return GPK_BAD_ARG;
  MomK k;
  GPK_TRY(mm_models(h, who, m, false, k));
  GPK_REQUIRE(h, M >= 1 && M <= GPK_SMALL_MAX_M, who + "M must be in [1, 32]");
  GPK_REQUIRE(h, Xq && mean && cov && xcov, who + "null pointer");
  GPK_REQUIRE(h, dXq && dSq, who + "null result dXq or dSq");
  const int D = k.D, nx = k.nx, NO = k.NO;
  const size_t n_q = (size_t)M * D, n_s = (size_t)M * nx * nx;
  const size_t n_om = (size_t)M * NO, n_oc = n_om * NO, n_ox = n_om * D;
  GPK_REQUIRE(h, gpk_finite(Xq, n_q), who + "the queries must not contain NaN or infinity");
  GPK_REQUIRE(h, !Sq || gpk_finite(Sq, n_s), who + "the covariances must not contain NaN or infinity");
  GPK_REQUIRE(h, (!gmean || gpk_finite(gmean, n_om)) && (!gcov || gpk_finite(gcov, n_oc)) && (!gxcov || gpk_finite(gxcov, n_ox)),
              who + "the seeds gmean, gcov and gxcov must not contain NaN or infinity");
  const MomWork sizes = mm_work(h, k, M, nullptr);
  const MomGradWork gsizes = mg_work(k, sizes, M, nullptr);
  const size_t n_up = n_q + n_s + n_om + n_oc + n_ox;
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, (n_up + n_om + n_oc + n_ox + n_q + n_s + sizes.doubles + gsizes.doubles) * sizeof(double), &ws));
  double* d_q = (double*)ws;
  double* d_S = d_q + n_q;
  double* d_gm = d_S + n_s;
  double* d_gc = d_gm + n_om;
  double* d_gx = d_gc + n_oc;
  double* d_om = d_gx + n_ox;
  double* d_oc = d_om + n_om;
  double* d_ox = d_oc + n_oc;
  double* d_dq = d_ox + n_ox;
  double* d_dS = d_dq + n_q;
  const MomWork w = mm_work(h, k, M, d_dS + n_s);
  const MomGradWork g = mg_work(k, w, M, d_dS + n_s + w.doubles);
  std::vector<double> host(n_up, 0.0);
  for (int r = 0; r < M; ++r) {
    for (int d = 0; d < D; ++d) {
      const double raw = Xq[(size_t)r * D + d];
      host[(size_t)r * D + d] = k.scaled ? (raw - k.in_shift[d]) / k.in_scale[d] : raw;
    }
    if (Sq)
      for (int i = 0; i < nx; ++i)
        for (int j = 0; j <= i; ++j)
          host[n_q + ((size_t)r * nx + i) * nx + j] = host[n_q + ((size_t)r * nx + j) * nx + i] = Sq[((size_t)r * nx + i) * nx + j];
  }
  if (gmean) memcpy(host.data() + n_q + n_s, gmean, sizeof(double) * n_om);
  if (gcov) memcpy(host.data() + n_q + n_s + n_om, gcov, sizeof(double) * n_oc);
  if (gxcov) memcpy(host.data() + n_q + n_s + n_om + n_oc, gxcov, sizeof(double) * n_ox);
  GPK_CHECK_HIP(h, hipMemcpyAsync(d_q, host.data(), sizeof(double) * n_up, hipMemcpyHostToDevice, h->stream));
  GPK_TRY(mm_launch(h, k, w, M, d_q, d_S));
  StageView v{};
  v.out[0] = d_om; v.out[1] = d_oc; v.out[2] = d_ox;
  mm_finish(h, k, w, v, M);
  GPK_LAUNCH_CHECK(h);
  mm_keep(h, k, w, M, g.keepE, g.keepF);
  GPK_LAUNCH_CHECK(h);
  const MomSeeds sd{d_gm, d_gc, d_gx, nullptr, nullptr, nullptr};
  GPK_TRY(mg_launch(h, k, w, g, M, d_q, sd, MomAdj{}, g.keepE, g.keepF, d_dq, d_dS));
  GPK_CHECK_HIP(h, hipMemcpyAsync(mean, d_om, sizeof(double) * n_om, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(cov, d_oc, sizeof(double) * n_oc, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(xcov, d_ox, sizeof(double) * n_ox, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(dXq, d_dq, sizeof(double) * n_q, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(dSq, d_dS, sizeof(double) * n_s, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  return GPK_OK;
}

// gpk_mm_chain with the backward sweep (z.grad).  Forward, per stage: the chain's five launches (traj, Sigma and the stage outputs
// keep their bits) and the keep launch; the scaled queries of every stage, E[mu] and the clip indicators stay in the device block,
// Sigma_h in the horizon's own output (Sigma_0: a second copy in the upload).  Backward, per stage: the forward's setup and row
// launches again (three) and the adjoint's four, the last of which makes the adjoint step.  Nothing of size N^2 or N R H is kept.
// One upload [head | S_0 | lam = gx_H | Lam = sym gS_H | gx | sym gS], 6 H + 7 H launches, one synchronisation.
// tape (the sparse entries ask for it; the exact ones do not): where H work blocks fit option moments_tape_mb, every stage's block
// (Sz, Bm, cm, G, cl, rowq, rowpart, pairpart) gets a region of its own, mm_work(h, k, R, tape + s w.doubles).  Forward, per stage:
// gpk_mm_chain's five launches and no keep launch.  Backward, per stage: the adjoint's four, the first of them
// moments_grad_setup_taped_kernel - nothing is recomputed.  5 H + 4 H launches; the buffers move and one reduction is fused in
// its order, no sum is reordered: every result has the bits of the sweep without the tape.
int gpk_mm_chain_grad(gpk_handle h, const std::string& who, const HostModels& m, const Horizon& z, bool tape) {
  if (!h) return GPK_BAD_ARG;
  MomK k;
  GPK_TRY(mm_models(h, who, m, true, k));
  GPK_TRY(gpk_horizon_check(h, who, k.nx, k.D, z));
  GPK_REQUIRE(h, z.grad, who + "null gradient block");
  const HorizonGrad& g = *z.grad;
  const int R = z.R, H = z.H, nx = k.nx, nu = k.D - k.nx;
  GPK_REQUIRE(h, g.gx && g.dx0, who + "null seed gx or null result dx0");
  GPK_REQUIRE(h, nu == 0 || g.dU, who + "null result dU");
  GPK_REQUIRE(h, gpk_finite(g.gx, (size_t)(H + 1) * R * nx) && (!g.gS || gpk_finite(g.gS, (size_t)(H + 1) * R * nx * nx)),
              who + "the seeds gx and gS must not contain NaN or infinity");
  const size_t n_om = (size_t)R * k.NO, n_du = (size_t)R * H * nu;
  HorizonBlock b(k.nx, k.D, z);
  const size_t n_x = b.n_x, n_s = b.n_s, n_Q = b.n_Q, n_gx = (size_t)H * n_x, n_gS = g.gS ? (size_t)H * n_s : 0;
  MomWork w = mm_work(h, k, R, nullptr);
  MomGradWork gw{};
  const bool taped = tape && h->moments_tape_mb > 0 && (size_t)H * w.doubles * sizeof(double) <= ((size_t)h->moments_tape_mb << 20);
  if (tape && h->gram_log)
    fprintf(stderr, "GPKMT tape%d h%d stage%zu launches%d\n", taped ? 1 : 0, H, w.doubles, (taped ? 9 : 13) * H);
  double *d_S0, *d_lam, *d_Lam, *d_gx, *d_gS, *d_kE, *d_kF, *d_du, *d_tape = nullptr;
  GPK_TRY(gpk_horizon_carve(h, b, [&] {
    b.head();
    d_S0 = b.take(n_s); d_lam = b.take(n_x); d_Lam = b.take(n_s); d_gx = b.take(n_gx); d_gS = b.take(n_gS);      // (uploaded)
    b.outputs(n_om, z.mean, n_om * k.NO, z.cov, n_om * k.D, z.xcov);
    b.qs = b.take((size_t)(H - 1) * b.n_q);
    d_kE = b.take(taped ? (size_t)0 : (size_t)H * R * 16);
    d_kF = b.take(taped ? (size_t)0 : (size_t)H * R * k.U);
    d_du = b.take(n_du);
    if (taped) {
      d_tape = b.take((size_t)H * w.doubles);
    } else {
      w = mm_work(h, k, R, b.base ? b.base + b.at : nullptr);
      b.take(w.doubles);
    }
    gw = mg_work(k, w, R, b.base ? b.base + b.at : nullptr);
    b.take(gw.doubles);
  }));
  std::vector<double> host(b.n_head() + n_s + n_x + n_s + n_gx + n_gS, 0.0);
  gpk_horizon_pack(b, z, k.scaled, k.in_shift, k.in_scale, host.data());
  double* hS0 = host.data() + b.n_head();
  double* hlam = hS0 + n_s;
  double* hLam = hlam + n_x;
  double* hgx = hLam + n_s;
  double* hgS = hgx + n_gx;
  memcpy(hS0, host.data() + n_x, sizeof(double) * n_s);
  memcpy(hlam, g.gx + (size_t)H * n_x, sizeof(double) * n_x);
  memcpy(hgx, g.gx, sizeof(double) * n_gx);
  if (g.gS) {
    // (gS + gS^T) / 2, the lower triangle formed and mirrored: stage H is the sweep's first Lam
    for (size_t t = 0; t < (size_t)(H + 1) * R; ++t) {
      const double* src = g.gS + t * n_Q;
      double* dst = t < (size_t)H * R ? hgS + t * n_Q : hLam + (t - (size_t)H * R) * n_Q;
      for (int i = 0; i < nx; ++i)
        for (int j = 0; j <= i; ++j) dst[i * nx + j] = dst[j * nx + i] = 0.5 * (src[i * nx + j] + src[j * nx + i]);
    }
  }
  GPK_TRY(gpk_horizon_upload(h, b, z, host));
  const MomSeeds sd{nullptr, nullptr, nullptr, d_lam, d_Lam, b.lin};
  if (taped) {
    for (int s = 0; s < H; ++s) {
      const MomWork ws = mm_work(h, k, R, d_tape + (size_t)s * w.doubles);
      GPK_TRY(mm_launch(h, k, ws, R, b.queries(s), b.S));
      gpk_time_begin(h, GPK_TIMED_PROPAGATE);
      mm_finish(h, k, ws, gpk_horizon_stage(b, z, s), R);
      gpk_time_end(h);
      GPK_LAUNCH_CHECK(h);
    }
    for (int s = H - 1; s >= 0; --s) {
      const MomWork ws = mm_work(h, k, R, d_tape + (size_t)s * w.doubles);
      const MomAdj ad{b.lin, d_gx + (size_t)s * n_x, g.gS ? d_gS + (size_t)s * n_s : nullptr, d_lam, d_Lam, d_du, H, s};
      GPK_TRY(mg_launch(h, k, ws, gw, R, b.queries(s), sd, ad, gw.keepE, nullptr, nullptr, nullptr, true));
    }
    return gpk_horizon_finish(h, b, z, {{g.dU, d_du, n_du}, {g.dx0, d_lam, n_x}, {g.dSigma0, d_Lam, n_s}});
  }
  for (int s = 0; s < H; ++s) {
    GPK_TRY(mm_launch(h, k, w, R, b.queries(s), b.S));
    gpk_time_begin(h, GPK_TIMED_PROPAGATE);
    mm_finish(h, k, w, gpk_horizon_stage(b, z, s), R);
    gpk_time_end(h);
    GPK_LAUNCH_CHECK(h);
    mm_keep(h, k, w, R, d_kE + (size_t)s * R * 16, d_kF + (size_t)s * R * k.U);
    GPK_LAUNCH_CHECK(h);
  }
  for (int s = H - 1; s >= 0; --s) {
    GPK_TRY(mm_launch_rows(h, k, w, R, b.queries(s), s == 0 ? d_S0 : b.sig + (size_t)(s - 1) * n_s));
    const MomAdj ad{b.lin, d_gx + (size_t)s * n_x, g.gS ? d_gS + (size_t)s * n_s : nullptr, d_lam, d_Lam, d_du, H, s};
    GPK_TRY(mg_launch(h, k, w, gw, R, b.queries(s), sd, ad, d_kE + (size_t)s * R * 16, d_kF + (size_t)s * R * k.U, nullptr, nullptr));
  }
  return gpk_horizon_finish(h, b, z, {{g.dU, d_du, n_du}, {g.dx0, d_lam, n_x}, {g.dSigma0, d_Lam, n_s}});
}

extern "C" int gpk_moments_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls, double sf2,
                                const double* y_mean, const double* y_std, const double* Kinv, int64_t Np, int64_t ldk, double kss,
                                double floor_, int var_includes_noise, double noise, int nx, const double* Xq, const double* Sq, int M,
                                double* mean, double* cov, double* xcov) {
  if (!h) return GPK_BAD_ARG;
  const HostModels m{1, P, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, &Kinv, Np, ldk, &kss, floor_, var_includes_noise, &noise, nx,
                    nullptr, nullptr, nullptr};
  GPK_REQUIRE(h, X && alpha, "moments_host: null pointer");
  GPK_REQUIRE(h, Kinv, "moments_host: null K^-1 (gpk_wtw of the model's inverse factor)");
  return gpk_mm_query(h, "moments_host: ", m, Xq, Sq, M, mean, cov, xcov);
}

extern "C" int gpk_moments_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                      const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                      const double* const* Kinv, int64_t Np, int64_t ldk, const double* kss, double floor_,
                                      int var_includes_noise, const double* noise, int nx, const double* in_shift,
                                      const double* in_scale, const double* Xq, const double* Sq, int M, double* mean, double* cov,
                                      double* xcov) {
  if (!h) return GPK_BAD_ARG;
  const HostModels m{B, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, Kinv, Np, ldk, kss, floor_, var_includes_noise, noise, nx,
                    nullptr, in_shift, in_scale};
  return gpk_mm_query(h, "moments_host_multi: ", m, Xq, Sq, M, mean, cov, xcov);
}

extern "C" int gpk_propagate_mm_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                     double sf2, const double* y_mean, const double* y_std, const double* Kinv, int64_t Np, int64_t ldk,
                                     double kss, double floor_, int var_includes_noise, double noise, const double* x0, int x0_rows,
                                     const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q,
                                     int R, int H, double* traj, double* Sigma, double* mean, double* cov, double* xcov) {
  if (!h) return GPK_BAD_ARG;
  const HostModels m{1, P, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, &Kinv, Np, ldk, &kss, floor_, var_includes_noise, &noise, P,
                    nullptr, nullptr, nullptr};
  GPK_REQUIRE(h, X && alpha, "propagate_mm_host: null pointer");
  GPK_REQUIRE(h, Kinv, "propagate_mm_host: null K^-1 (gpk_wtw of the model's inverse factor)");
  GPK_REQUIRE(h, P >= 1 && P <= D, "propagate_mm_host: the state dimension P must be in [1, 16] and must not exceed D");
  Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean};
  z.cov = cov; z.xcov = xcov;
  return gpk_mm_chain(h, "propagate_mm_host: ", m, z);
}

extern "C" int gpk_propagate_mm_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                           const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                           const double* const* Kinv, int64_t Np, int64_t ldk, const double* kss, double floor_,
                                           int var_includes_noise, const double* noise, int nx, const int* coord,
                                           const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                           const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                           const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* cov,
                                           double* xcov) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, coord, "propagate_mm_host_multi: null pointer");
  const HostModels m{B, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, Kinv, Np, ldk, kss, floor_, var_includes_noise, noise, nx, coord,
                    in_shift, in_scale};
  Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean};
  z.cov = cov; z.xcov = xcov;
  return gpk_mm_chain(h, "propagate_mm_host_multi: ", m, z);
}

// ... with the adjoint: the seeds gmean (M x NO), gcov (M x NO x NO; (g + g^T) / 2 is used) and gxcov (M x NO x D, columns >= nx
// ignored), null: zero; the results dXq (M x D) and dSq (M x nx x nx)
extern "C" int gpk_moments_vjp_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                    double sf2, const double* y_mean, const double* y_std, const double* Kinv, int64_t Np, int64_t ldk,
                                    double kss, double floor_, int var_includes_noise, double noise, int nx, const double* Xq,
                                    const double* Sq, int M, double* mean, double* cov, double* xcov, const double* gmean,
                                    const double* gcov, const double* gxcov, double* dXq, double* dSq) {
  if (!h) return GPK_BAD_ARG;
  const HostModels m{1, P, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, &Kinv, Np, ldk, &kss, floor_, var_includes_noise, &noise, nx,
                    nullptr, nullptr, nullptr};
  GPK_REQUIRE(h, X && alpha, "moments_vjp_host: null pointer");
  GPK_REQUIRE(h, Kinv, "moments_vjp_host: null K^-1 (gpk_wtw of the model's inverse factor)");
  return gpk_mm_query_vjp(h, "moments_vjp_host: ", m, Xq, Sq, M, mean, cov, xcov, gmean, gcov, gxcov, dXq, dSq);
}

extern "C" int gpk_moments_vjp_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                          const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                          const double* const* Kinv, int64_t Np, int64_t ldk, const double* kss, double floor_,
                                          int var_includes_noise, const double* noise, int nx, const double* in_shift,
                                          const double* in_scale, const double* Xq, const double* Sq, int M, double* mean, double* cov,
                                          double* xcov, const double* gmean, const double* gcov, const double* gxcov, double* dXq,
                                          double* dSq) {
  if (!h) return GPK_BAD_ARG;
  const HostModels m{B, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, Kinv, Np, ldk, kss, floor_, var_includes_noise, noise, nx,
                    nullptr, in_shift, in_scale};
  return gpk_mm_query_vjp(h, "moments_vjp_host_multi: ", m, Xq, Sq, M, mean, cov, xcov, gmean, gcov, gxcov, dXq, dSq);
}

// ... with the gradient of a horizon cost: the seeds gx, gS and the results dU, dx0, dSigma0 as HorizonGrad describes them
extern "C" int gpk_propagate_mm_grad_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                          double sf2, const double* y_mean, const double* y_std, const double* Kinv, int64_t Np,
                                          int64_t ldk, double kss, double floor_, int var_includes_noise, double noise,
                                          const double* x0, int x0_rows, const double* U, int u_rows, const double* lin,
                                          const double* Sigma0, int s_rows, const double* Q, int R, int H, double* traj, double* Sigma,
                                          double* mean, double* cov, double* xcov, const double* gx, const double* gS, double* dU,
                                          double* dx0, double* dSigma0) {
  if (!h) return GPK_BAD_ARG;
  const HostModels m{1, P, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, &Kinv, Np, ldk, &kss, floor_, var_includes_noise, &noise, P,
                    nullptr, nullptr, nullptr};
  GPK_REQUIRE(h, X && alpha, "propagate_mm_grad_host: null pointer");
  GPK_REQUIRE(h, Kinv, "propagate_mm_grad_host: null K^-1 (gpk_wtw of the model's inverse factor)");
  GPK_REQUIRE(h, P >= 1 && P <= D, "propagate_mm_grad_host: the state dimension P must be in [1, 16] and must not exceed D");
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean};
  z.cov = cov; z.xcov = xcov; z.grad = &g;
  return gpk_mm_chain_grad(h, "propagate_mm_grad_host: ", m, z);
}

extern "C" int gpk_propagate_mm_grad_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                                int D, const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                                const double* const* Kinv, int64_t Np, int64_t ldk, const double* kss, double floor_,
                                                int var_includes_noise, const double* noise, int nx, const int* coord,
                                                const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                                const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                                const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* cov,
                                                double* xcov, const double* gx, const double* gS, double* dU, double* dx0,
                                                double* dSigma0) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, coord, "propagate_mm_grad_host_multi: null pointer");
  const HostModels m{B, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, Kinv, Np, ldk, kss, floor_, var_includes_noise, noise, nx, coord,
                    in_shift, in_scale};
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean};
  z.cov = cov; z.xcov = xcov; z.grad = &g;
  return gpk_mm_chain_grad(h, "propagate_mm_grad_host_multi: ", m, z);
}
