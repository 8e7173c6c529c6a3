// K9: sparse inducing-point GP (Titsias / DTC "projected process" predictor, the form of GPflow's SGPR) - fit on every row,
// serve through m inducing inputs Z.
//
// The training rows enter through ADDITIVE fp64 statistics of size m x m, kept as ONE symmetric matrix
//   S = F^T F,  F = [Kfu | Yn]  (rows x (mp + 128); mp = m rounded up to 128; zero in the padding)
//   S[0:mp, 0:mp] = G = Kuf Kfu,   S[mp + p, 0:mp] = g[:, p] = Kuf Yn[:, p],   S[mp + p, mp + q] = Yn[:, p] . Yn[:, q]
// so that appending rows is S += F_new^T F_new.  The statistics pass is this file's hot path (N m^2 flops):
//   per panel of rows   sparse_panel_kernel   F (exact differences of the length-scale-divided coordinates, as
//                                             gpk_cross_gram_t; the normalised targets ride in the last 128 columns)
//                       tile GEMM             the lower tiles of F^T F on the fp64 matrix cores.  The product is tall and
//                                             skinny (m = 1024: 45 lower 128-tiles for 256 CUs), so the panel's rows are cut
//                                             into `slabs` k-slabs, each an independent product of the GEMM's explicit batch
//                                             mode writing its own partial matrix ...
//                       sparse_reduce_kernel  ... which are added IN SLAB ORDER into S and mirrored to both halves: no
//                                             floating-point atomics, the same sequence of updates gives the same bits.
//   One slab: the GEMM accumulates straight into the lower tiles of S (beta = 1) and one mirror pass ends the call.
// The slab count depends on (mp, panel rows) only (sparse_slabs_for), overridable by option "sparse_slabs"; the panel by
// option "sparse_panel" (sparse_panel_for: F within half of the 256 MB Infinity Cache).
//
// FITC (gpk_sparse_set_approximation): the other standard inducing-point posterior differs in the statistics only, S = F^T diag(w) F
// with w_i = s2 / (s2 + max(sf2 - |Wuu k_u(x_i)|^2, 0)).  The weighted pass (`accumulate` with FitcArgs) adds three launches per
// panel between the panel kernel and the F^T F launches: the q_i (gpk_predict_var_inv's tile GEMM with the panel as its second
// operand, V never stored), sparse_fitc_scale_kernel (lambda, w, F scaled by sqrt(w) in place, partial sums of log lambda) and
// the fixed-order sum of those onto the running sum_i log lambda_i, the likelihood's one extra scalar.  The assembly and
// everything that serves the assembled model are the same code for both kinds.
//
// Training (gpk_sparse_hold / gpk_sparse_eval): the rows stay on the device, an evaluation accumulates S again, assembles the
// model and, for the gradient of the bound, runs ONE more pass over the rows (rows_pass: F again, a tile GEMM Q = F C whose
// epilogue reduces Q o Kfu o ((x - z) / ls)^2 per tile without storing Q, a fixed-order sum of the tiles); the m x m part is
// gpk_wtw, tile GEMMs and gpk_lml_grad's pass on Z.  gpk_sparse_eval_z also moves Z and differentiates with respect to it: the
// same loop once more with the epilogue that reduces Q o Kfu o (x - z) / ls per column, and sparse_kuu_z_kernel for the Kuu
// term.  include/gpk.h has the formulas.
//
// The assembly (gpk_sparse_finalize) is host code over entries that exist: gpk_gram / gpk_potrf / gpk_trtri, tile GEMMs with
// triangular k-ranges, gpk_lml_terms.  The serving (gpk_sparse_predict, gpk_sparse_predict_grad, gpk_sparse_predict_cov): up to
// 32 queries the two-factor form of the small-batch kernels (gpk_small.hip, through the serving routines of gpk_serve.hip: one
// K*, P outputs, the inverse factors Wuu and WSigma as a grid dimension, combined by the last workgroup); larger batches the
// query-panel loop (gpk_compose.h, shared with gpk_model.hip and gpk_bmodel.hip) over gpk_predict_mean, gpk_predict_var_inv,
// gpk_predict_mean_grad and gpk_predict_var_grad_inv once per factor with a small combining launch, and for the covariance the
// stacked panel [Wuu K*; WSigma K*] with ONE symmetric tile GEMM.  The buffers are gpk_dev members of the object.  DESIGN.md, K9.
#include <cfloat>

#include "gpk_compose.h"
#include "gpk_math.h"

namespace {

constexpr int NB = GPK_TILE;
constexpr int SP_TS = 64;             // sparse_panel_kernel: rows x columns of F per workgroup
constexpr int SP_MAX_SLABS = 64;
constexpr int64_t SP_MAX_M = 16384;   // inducing inputs (the small-batch serving kernels' limit on the padded size)

struct SpLs { double v[GPK_MAX_D_PREDICT]; };
struct SpP { double v[GPK_MAX_P]; };

// F[i][j] = sf2 exp(-0.5 |(x_i - z_j) / ls|^2) for i < n, j < m;  F[i][mp + p] = Yn[i][p] for i < n, p < P;  0 elsewhere in
// the (gridDim.y * 64) x (mp + 128) block.  64 x 64 entries per workgroup, a 4 x 4 micro-tile per thread whose columns are
// the two pairs {2 tx, 2 tx + 1} and {32 + 2 tx, 33 + 2 tx}: every 16-byte store of 16 neighbouring lanes covers 256
// contiguous bytes.  D <= 16: rows and inducing inputs are staged once, divided by the length-scales.
__global__ __launch_bounds__(256) void sparse_panel_kernel(const double* __restrict__ X, const double* __restrict__ Yn,
                                                           long long n, const double* __restrict__ Z, int m, int D, int P,
                                                           SpLs ls, double sf2, double* __restrict__ F, long long ldf,
                                                           int mp) {
  __shared__ __attribute__((aligned(16))) double xi[GPK_MAX_D_PREDICT * SP_TS];
  __shared__ __attribute__((aligned(16))) double zj[GPK_MAX_D_PREDICT * SP_TS];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long i0 = (long long)blockIdx.y * SP_TS;
  const int j0 = blockIdx.x * SP_TS;
  if (j0 >= mp) {      // the targets' 128 columns
    for (int e = tid; e < SP_TS * SP_TS; e += 256) {
      const int r = e >> 6, c = e & 63, p = j0 - mp + c;
      const long long gi = i0 + r;
      F[gi * ldf + j0 + c] = (gi < n && p < P) ? Yn[gi * P + p] : 0.0;
    }
    return;
  }
  for (int e = tid; e < SP_TS * D; e += 256) {
    const int i = e / D, d = e - i * D;
    const long long gi = i0 + i;
    const int gj = j0 + i;
    xi[d * SP_TS + i] = gi < n ? X[gi * D + d] / ls.v[d] : 0.0;
    zj[d * SP_TS + i] = gj < m ? Z[(long long)gj * D + d] / ls.v[d] : 0.0;
  }
  __syncthreads();
  double d2[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) d2[r][c] = 0.0;
  for (int d = 0; d < D; ++d) {
    double a[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = xi[d * SP_TS + 4 * ty + r];
#pragma unroll
    for (int c = 0; c < 4; ++c) b[c] = zj[d * SP_TS + (c >> 1) * 32 + 2 * tx + (c & 1)];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double df = a[r] - b[c];
        d2[r][c] = __builtin_fma(df, df, d2[r][c]);
      }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long gi = i0 + 4 * ty + r;
    double v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int gj = j0 + (c >> 1) * 32 + 2 * tx + (c & 1);
      v[c] = (gi < n && gj < m) ? sf2 * gpk_exp_neg(-0.5 * d2[r][c]) : 0.0;
    }
    double* row = F + gi * ldf + j0 + 2 * tx;
    *reinterpret_cast<double2*>(row) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(row + 32) = make_double2(v[2], v[3]);
  }
}

// S[i][j] = S[j][i] = S[i][j] + sum_{s < nslabs, in slab order} partial[s][i][j] for i >= j (nt x nt, 32 x 32 entries per
// workgroup over the lower triangle; the transposed half goes through LDS so that both stores are contiguous).  nslabs == 0:
// the mirror alone.  Only entries i >= j of S and of the partials are read.
__global__ __launch_bounds__(256) void sparse_reduce_kernel(double* __restrict__ S, long long ld,
                                                            const double* __restrict__ partial, int nslabs,
                                                            long long pstride, int nt) {
  __shared__ double t[32][33];
  const long long id = blockIdx.x;
  long long bi = (long long)((__builtin_sqrt(8.0 * (double)id + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= id) ++bi;
  while (bi * (bi + 1) / 2 > id) --bi;
  const long long bj = id - bi * (bi + 1) / 2;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int li = ty + 8 * r;
    const long long i = bi * 32 + li, j = bj * 32 + tx;
    if (i >= j) {
      double v = S[i * ld + j];
      for (int s = 0; s < nslabs; ++s) v += partial[s * pstride + i * nt + j];
      S[i * ld + j] = v;
      t[li][tx] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int li = ty + 8 * r;
    const long long gi = bj * 32 + li, gj = bi * 32 + tx;
    if (gj > gi) S[gi * ld + gj] = t[tx][li];
  }
}

// out[0] = sum_{i < mp} B[i][i] (= tr(Wuu G Wuu^T) / sigma^2, added in a fixed order), then B[i][i] += 1;
// out[1 + p] = S[mp + p][mp + p] = yy[p].  One workgroup.
__global__ __launch_bounds__(256) void sparse_diag_kernel(double* __restrict__ B, long long ldb, int mp,
                                                          const double* __restrict__ S, long long lds_, int P,
                                                          double* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < mp; i += 256) {
    const double v = B[(long long)i * ldb + i];
    s += v;
    B[(long long)i * ldb + i] = v + 1.0;
  }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[0] = red[0];
  if (tid < P) out[1 + tid] = S[(long long)(mp + tid) * lds_ + mp + tid];
}

// the first P columns of three (m x 128) panels as compact (m x P) arrays
__global__ void sparse_unpack_kernel(const double* __restrict__ p0, const double* __restrict__ p1,
                                     const double* __restrict__ p2, long long m, int P, double* __restrict__ o0,
                                     double* __restrict__ o1, double* __restrict__ o2) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= m * P) return;
  const long long i = e / P;
  const int p = (int)(e - i * P);
  o0[e] = p0[i * NB + p];
  o1[e] = p1[i * NB + p];
  o2[e] = p2[i * NB + p];
}

// out[i][p] = max(v0[i] - v1[i], floor) y_std[p]^2   (v0 = kss - |Wuu k|^2, v1 = -|WSigma k|^2)
__global__ void sparse_var_kernel(const double* __restrict__ v0, const double* __restrict__ v1, long long M, int P, SpP ys,
                                  double floor_, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * P) return;
  const long long i = e / P;
  const int p = (int)(e - i * P);
  out[e] = fmax(v0[i] - v1[i], floor_) * ys.v[p] * ys.v[p];
}

// the gradient panels' counterpart: var[i][p] as above and dvar[i][p][d] = (g0[i][d] - g1[i][d]) y_std[p]^2
// (g0 = d/dx (kss - |Wuu k|^2), g1 = d/dx (-|WSigma k|^2), both unclipped)
__global__ void sparse_var_grad_kernel(const double* __restrict__ v0, const double* __restrict__ v1, const double* __restrict__ g0,
                                       const double* __restrict__ g1, long long M, int P, int D, SpP ys, double floor_,
                                       double* __restrict__ var, double* __restrict__ dvar) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * P * D) return;
  const long long ip = e / D, i = ip / P;
  const int d = (int)(e - ip * D), p = (int)(ip - i * P);
  dvar[e] = (g0[i * D + d] - g1[i * D + d]) * (ys.v[p] * ys.v[p]);
  if (d == 0) var[ip] = fmax(v0[i] - v1[i], floor_) * ys.v[p] * ys.v[p];
}

// the second operand of the covariance product: rows < mp of the stacked panel [V0; V1] as they are, rows >= mp negated
__global__ void sparse_stack_kernel(const double* __restrict__ VA, long long mp, long long cols, double* __restrict__ VB) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * mp * cols) return;
  VB[e] = e < mp * cols ? VA[e] : -VA[e];
}

int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// FITC ("FITC"): the weights of a panel's rows and the scaled panel, one launch.  Per 64-row block (blockIdx.y) the
// first 64 threads form, for the row i < n,
//   q_i = |Wuu k_u(x_i)|^2 = sum over the ntm tile rows of qpart[t * ldq + i], added in tile order (epilogue 1 of the tile GEMM
//         Wuu F^T left one sum of squares per tile row) - or, ntm == 0, resid[i] = sf2 - q_i as gpk_predict_var_inv left it,
//   lambda_i = s2 + max(sf2 - q_i, 0),   w_i = s2 / lambda_i in (0, 1],
// then the workgroup multiplies its rows of F, columns [1024 blockIdx.x, + 1024) of all nt (Kfu and the targets), by
// sqrt(w_i) in place; the column-0 workgroup writes logpart[blockIdx.y] = sum of log lambda_i over its rows, in row order, and
// wout[i] = w_i where wout != NULL.  Rows >= n of the last block are zero and stay zero, and contribute no logarithm.
__global__ __launch_bounds__(256) void sparse_fitc_scale_kernel(double* __restrict__ F, long long ldf, int nt, long long n,
                                                                const double* __restrict__ qpart, int ntm, long long ldq,
                                                                const double* __restrict__ resid, double sf2, double s2,
                                                                double* __restrict__ logpart, double* __restrict__ wout) {
  __shared__ double sw[SP_TS], lg[SP_TS];
  const int tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.y * SP_TS;
  if (tid < SP_TS) {
    const long long i = i0 + tid;
    double w = 0.0, l = 0.0;
    if (i < n) {
      double r;
      if (ntm > 0) {
        double q = 0.0;
        for (int t = 0; t < ntm; ++t) q += qpart[(long long)t * ldq + i];
        r = sf2 - q;
      } else {
        r = resid[i];
      }
      const double lam = s2 + fmax(r, 0.0);
      const double wi = s2 / lam;
      w = __builtin_sqrt(wi);
      l = log(lam);
      if (wout && blockIdx.x == 0) wout[i] = wi;
    }
    sw[tid] = w;
    lg[tid] = l;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) {
    double t = 0.0;
    for (int r = 0; r < SP_TS; ++r) t += lg[r];
    logpart[blockIdx.y] = t;
  }
  const int c0 = blockIdx.x * 1024, c1 = c0 + 1024 < nt ? c0 + 1024 : nt;
  for (int r = tid >> 6; r < SP_TS; r += 4) {
    const double w = sw[r];
    double* row = F + (i0 + r) * ldf;
    for (int c = c0 + 2 * (tid & 63); c < c1; c += 128) {
      double2 v = *reinterpret_cast<double2*>(row + c);
      v.x *= w;
      v.y *= w;
      *reinterpret_cast<double2*>(row + c) = v;
    }
  }
}

__global__ void sparse_sum_kernel(const double* __restrict__ partial, long long n, int W, double* __restrict__ out, int accumulate);

// what the weighted pass takes beside the plain one's operands: the inverse factor Wuu (dev, mp x ldw, gpk_trtri's layout),
// s2 = noise + jitter, loglam (dev double[1]: += sum log lambda_i), wout (dev n doubles or NULL: the weights)
struct FitcArgs { const double* Wuu; int64_t ldw; double s2; double* loglam; double* wout; };

// Rows of a panel: F = rows x (mp + 128) doubles within 128 MiB - half of the 256 MB Infinity Cache, so that the panel the
// cross kernel has just written is still on the chip while the (mp / 128 + 1) tile columns of the product read it again -
// between 1024 and 16384 rows, a multiple of 256.  Measured (N = 262 144, ms at 2048 / 4096 / 8192 / 16384 rows,
// profiles/r11_exp_sparse_second_rule.log): m = 256 4.75 / 3.10 / 2.28 / 1.72 and m = 1024 12.09 / 9.33 / 7.92 / 7.18 (F = 50 /
// 151 MB at 16384 rows: the longer panel wins), m = 4096 with one slab 94.5 / 94.0 / 96.2 / 107.6 (F = 138 MB at 4096 rows, 554 MB
// at 16384: it falls out of the cache).  Option "sparse_panel" overrides.
int64_t sparse_panel_for(gpk_handle h, int64_t mp) {
  if (h->sparse_panel > 0) return h->sparse_panel;
  int64_t rows = (int64_t)((128ll << 20) / ((mp + NB) * 8)) / 256 * 256;
  if (rows > 16384) rows = 16384;
  if (rows < 1024) rows = 1024;
  return rows;
}

// k-slabs of a panel's product: a function of (mp, rows) only.  From 256 lower 128-tiles on (the CU count) one product
// fills the chip: ONE slab, accumulated straight into S.  Below that, the fewest slabs that bring the launch to 1024 tiles
// (two rounds of the 512 resident workgroups, from where on the tile GEMM keeps its 128 x 128 tiles), at most 16, never
// slabs of fewer than 512 rows.  Measured (profiles/r11_exp_sparse_first_rule.log; ms at 1 / 2 / 4 / 8 / 16 / 32 slabs): m = 256 (6 tiles) 4.92 / 3.07 / 2.21 /
// 1.70 / 1.71 / 1.96, m = 1024 (45 tiles) 9.98 / 9.42 / 9.19 / 7.72 / 7.40 / 8.62, m = 4096 (561 tiles) 96.7 / 125.4 / 129.0 /
// 147.4 / 167.1 / 203.7 - there every slab is a pass over a 143 MB partial matrix and buys nothing.  Option "sparse_slabs"
// overrides (1 .. 64).
int sparse_slabs_for(gpk_handle h, int64_t mp, int64_t rows) {
  if (h->sparse_slabs > 0) return h->sparse_slabs < SP_MAX_SLABS ? h->sparse_slabs : SP_MAX_SLABS;
  const int64_t T = mp / NB + 1, tiles = T * (T + 1) / 2;
  if (tiles >= 256) return 1;
  int64_t s = (1024 + tiles - 1) / tiles;
  if (s > 16) s = 16;
  if (s > rows / 512) s = rows / 512;
  return s < 1 ? 1 : (int)s;
}

struct PanelPlan { int slabs; int64_t slab_rows, rows_p; };
PanelPlan plan_panel(gpk_handle h, int64_t mp, int64_t rows) {
  PanelPlan p;
  p.slabs = sparse_slabs_for(h, mp, rows);
  p.slab_rows = round_up((rows + p.slabs - 1) / p.slabs, SP_TS);
  p.rows_p = p.slab_rows * p.slabs;
  return p;
}

// S (nt x ld, nt = mp + 128; symmetric on entry and on return) += F^T F over the n rows of X / Yn, panel by panel.
// fitc != NULL: the weighted pass, S += F^T diag(w) F.  Per panel, between the panel kernel and the F^T F launches that run
// unchanged on the scaled panel: the q_i (option "fitc_fused" = 1: ONE tile GEMM Wuu F[:, 0:mp]^T whose epilogue 1 keeps only
// the sums of squares per tile row - gpk_predict_var_inv's launch with the panel in the place of a second kernel matrix; 0:
// gpk_predict_var_inv itself on the panel's rows, the composed route kept as the check of the fused one), the scaling launch,
// and the sum of the workgroups' log lambda onto fitc->loglam.  The panel is written in whole 128-row blocks (the GEMM's n).
// Work area: [the head that gpk_predict_var_inv's own request lands in (unfused) | F | partial | the q work | log partials].
int accumulate(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m, int D, int P,
               const double* ls, double sf2, double* S, int64_t ld, const FitcArgs* fitc = nullptr) {
  const int64_t mp = gpk_padded(m), nt = mp + NB;
  SpLs l;
  for (int d = 0; d < D; ++d) {
    GPK_REQUIRE(h, ls[d] > 0.0 && std::isfinite(ls[d]), "sparse: length-scales must be positive");
    l.v[d] = ls[d];
  }
  const int64_t panel = sparse_panel_for(h, mp);
  // the work area: F for the largest panel and the partial products of the launch with the most slabs
  int64_t f_rows = 0, max_slabs = 0;
  const int64_t last = n - (n - 1) / panel * panel;       // rows of the last panel; the others are full
  for (const int64_t rows : {n < panel ? n : panel, last}) {
    const PanelPlan p = plan_panel(h, mp, rows);
    if (p.rows_p > f_rows) f_rows = p.rows_p;
    if (p.slabs > 1 && p.slabs > max_slabs) max_slabs = p.slabs;
  }
  const bool fused = fitc && h->fitc_fused;
  size_t head = 0, qwork = 0;
  if (fitc) {
    f_rows = round_up(f_rows, NB);
    const size_t qpart = (size_t)(mp / 64) * f_rows;      // one sum of squares per (64-row tile row of Wuu, row of the panel)
    if (!fused) head = qpart;
    qwork = (fused ? qpart : (size_t)f_rows * mp + f_rows) + (size_t)(f_rows / SP_TS);
  }
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, (head + (size_t)f_rows * nt + (size_t)max_slabs * nt * nt + qwork) * sizeof(double), &ws));
  double* F = (double*)ws + head;
  double* partial = F + (size_t)f_rows * nt;
  double* qw = partial + (size_t)max_slabs * nt * nt;
  const unsigned nb32 = (unsigned)(nt / 32);
  const unsigned red_blocks = nb32 * (nb32 + 1) / 2;
  bool direct = false;
  for (int64_t r0 = 0; r0 < n; r0 += panel) {
    const int64_t nr = n - r0 < panel ? n - r0 : panel;
    const PanelPlan p = plan_panel(h, mp, nr);
    const int64_t rows_w = fitc ? round_up(p.rows_p, NB) : p.rows_p;
    hipLaunchKernelGGL(sparse_panel_kernel, dim3((unsigned)(nt / SP_TS), (unsigned)(rows_w / SP_TS)), dim3(256), 0,
                       h->stream, X + r0 * D, Yn + r0 * P, (long long)nr, Z, (int)m, D, P, l, sf2, F, (long long)nt,
                       (int)mp);
    GPK_LAUNCH_CHECK(h);
    if (fitc) {
      const unsigned nblk = (unsigned)(p.rows_p / SP_TS);
      double* logpart = qw + (fused ? (size_t)(mp / 64) * f_rows : (size_t)f_rows * mp + f_rows);
      int ntm = 0;
      const double* resid = nullptr;
      if (fused) {
        // V = Wuu F[:, 0:mp]^T tile by tile (Wuu lower: k < row-tile end), never stored: qw[tile_row][i]
        GemmArgs g = gemm_args(fitc->Wuu, fitc->ldw, 0, F, nt, 0, qw, rows_w, (int)mp, (int)rows_w, (int)mp, 1.0, 0.0);
        g.ke0 = NB; g.ke_row = NB; g.epilogue = 1; g.k_super = 1; g.heavy_first = 1;
        ntm = (int)(mp / gpk_gemm_tile(h, g));
        GPK_TRY(gpk_gemm(h, GPK_F64, g));
      } else {
        // (its request for the handle's scratch is smaller than this call's and returns the same block: the head)
        double* var = qw + (size_t)f_rows * mp;
        GPK_TRY(gpk_predict_var_inv(h, GPK_F64, Z, m, D, ls, sf2, fitc->Wuu, mp, fitc->ldw, X + r0 * D, nr, sf2,
                                    -std::numeric_limits<double>::max(), qw, var));
        resid = var;
      }
      hipLaunchKernelGGL(sparse_fitc_scale_kernel, dim3((unsigned)((nt + 1023) / 1024), nblk), dim3(256), 0, h->stream, F,
                         (long long)nt, (int)nt, (long long)nr, (const double*)qw, ntm, (long long)rows_w, resid, sf2, fitc->s2,
                         logpart, fitc->wout ? fitc->wout + r0 : nullptr);
      GPK_LAUNCH_CHECK(h);
      hipLaunchKernelGGL(sparse_sum_kernel, dim3(1), dim3(256), 0, h->stream, (const double*)logpart, (long long)nblk, 1,
                         fitc->loglam, 1);
      GPK_LAUNCH_CHECK(h);
    }
    if (p.slabs > 1) {
      GemmArgs g = gemm_args(F, nt, 1, F, nt, 1, partial, nt, (int)nt, (int)nt, (int)p.slab_rows, 1.0, 0.0);
      g.lower_only = 1;
      g.nbatch = p.slabs;
      g.sA = g.sB = (long long)p.slab_rows * nt * 8;
      g.sC = (long long)nt * nt * 8;
      GPK_TRY(gpk_gemm(h, GPK_F64, g));
      hipLaunchKernelGGL(sparse_reduce_kernel, dim3(red_blocks), dim3(256), 0, h->stream, S, (long long)ld, partial,
                         p.slabs, (long long)nt * nt, (int)nt);
      GPK_LAUNCH_CHECK(h);
    } else {
      GemmArgs g = gemm_args(F, nt, 1, F, nt, 1, S, ld, (int)nt, (int)nt, (int)p.slab_rows, 1.0, 1.0);
      g.lower_only = 1;
      GPK_TRY(gpk_gemm(h, GPK_F64, g));
      direct = true;
    }
  }
  if (direct) {
    hipLaunchKernelGGL(sparse_reduce_kernel, dim3(red_blocks), dim3(256), 0, h->stream, S, (long long)ld, partial, 0,
                       (long long)nt * nt, (int)nt);
    GPK_LAUNCH_CHECK(h);
  }
  return GPK_OK;
}

// out[c] (+)= sum_{b < n} partial[b * W + c]: one workgroup per component, a fixed-order strided sum and a tree (as
// grad_reduce_kernel); accumulate != 0 adds to what out[c] holds (the running sums of the row pass, panel after panel)
__global__ __launch_bounds__(256) void sparse_sum_kernel(const double* __restrict__ partial, long long n, int W,
                                                         double* __restrict__ out, int accumulate) {
  __shared__ double red[256];
  const int c = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (long long b = tid; b < n; b += 256) s += partial[b * W + c];
  red[tid] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[c] = accumulate ? out[c] + red[0] : red[0];
}

// The coefficient matrix of the row pass and the matrix of the Kuu term, from Ki = Kuu^-1, Si = Sigma~ (both full, mp x mp),
// M3 = Kuu^-1 G Kuu^-1 (lower tiles) and alpha_u (m x P):
//   Cm[i][j] = (P / s2) (Ki - Si)_ij - alpha_i . alpha_j / s2  (i, j < m),  Cm[mp + p][j] = alpha_jp / s2  (p < P, j < m),  0 elsewhere
//   M3[i][j] <- (Ki - Si)_ij - M3_ij / s2                      (the lower tiles, in place)
__global__ __launch_bounds__(256) void sparse_coef_kernel(const double* __restrict__ Ki, const double* __restrict__ Si,
                                                          double* __restrict__ M3, const double* __restrict__ alpha, int m,
                                                          int mp, int P, double is2, double* __restrict__ Cm) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)(mp + NB) * mp) return;
  const int i = (int)(e / mp), j = (int)(e - (long long)i * mp);
  double v = 0.0;
  if (i < mp) {
    const double df = Ki[e] - Si[e];
    if (i < m && j < m) {
      double aa = 0.0;
      for (int p = 0; p < P; ++p) aa = __builtin_fma(alpha[(long long)i * P + p], alpha[(long long)j * P + p], aa);
      v = (double)P * is2 * df - aa * is2;
    }
    if (i / NB >= j / NB) M3[e] = df - M3[e] * is2;
  } else if (i - mp < P && j < m) {
    v = alpha[(long long)j * P + (i - mp)] * is2;
  }
  Cm[e] = v;
}

// part[i][0 .. 3] for the inducing input i < m (one workgroup each): sum_j Ki_ij G_ij, sum_j Si_ij G_ij, alpha_i . g_i,
// alpha_i . (G alpha)_i;  G and g are blocks of S (leading dimension lds_), GA = G alpha is an (mp x 128) panel
__global__ __launch_bounds__(256) void sparse_dots_kernel(const double* __restrict__ Ki, const double* __restrict__ Si,
                                                          const double* __restrict__ S, long long lds_, const double* __restrict__ alpha,
                                                          const double* __restrict__ GA, int m, int mp, int P,
                                                          double* __restrict__ part) {
  __shared__ double red[2][256];
  const int i = blockIdx.x, tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int j = tid; j < m; j += 256) {
    const double g = S[(long long)i * lds_ + j];
    a = __builtin_fma(Ki[(long long)i * mp + j], g, a);
    b = __builtin_fma(Si[(long long)i * mp + j], g, b);
  }
  red[0][tid] = a;
  red[1][tid] = b;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { red[0][tid] += red[0][tid + off]; red[1][tid] += red[1][tid + off]; }
    __syncthreads();
  }
  if (tid == 0) {
    double c = 0.0, d = 0.0;
    for (int p = 0; p < P; ++p) {
      const double al = alpha[(long long)i * P + p];
      c = __builtin_fma(al, S[(long long)i * lds_ + mp + p], c);
      d = __builtin_fma(al, GA[(long long)i * NB + p], d);
    }
    part[4 * i] = red[0][0];
    part[4 * i + 1] = red[1][0];
    part[4 * i + 2] = c;
    part[4 * i + 3] = d;
  }
}

// R[c][w] (+)= sum over the tile rows tm, in tile order, of the column sums of epilogue 5,
// partial[((tm * ntn + c / ts) * ts + c % ts) * GPK_GRAD_W + w]: 64 entries of R per workgroup, four interleaved strided sums
// each and a fixed-order sum of the four; accumulate != 0 adds to what R holds (panel after panel)
__global__ __launch_bounds__(256) void sparse_colsum_kernel(const double* __restrict__ partial, int ntm, int ntn, int ts,
                                                            double* __restrict__ R, int accumulate) {
  __shared__ double red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long long e = (long long)blockIdx.x * 64 + tx;        // (mp * GPK_GRAD_W is a multiple of 64)
  const int c = (int)(e / GPK_GRAD_W), w = (int)(e - (long long)c * GPK_GRAD_W);
  const int tn = c / ts, cl = c - tn * ts;
  double s = 0.0;
  for (int tm = ty; tm < ntm; tm += 4) s += partial[(((long long)tm * ntn + tn) * ts + cl) * GPK_GRAD_W + w];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0) {
    const double v = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    R[e] = accumulate ? R[e] + v : v;
  }
}

// V[i][d] = 2 sum_j GammaK_ij Kuu0_ij (z_jd / ls_d - z_id / ls_d) for d < D, GammaK_ij = (P / 2) M_ij - alpha_i . alpha_j / 2,
// Kuu0_ij = sf2 exp(-0.5 |(z_i - z_j) / ls|^2) recomputed by exact differences of the divided coordinates (as
// sparse_panel_kernel): the inducing input i < m per workgroup, M = Kuu^-1 - Sigma~ - Kuu^-1 G Kuu^-1 / s2 full (ld = mp), thread t
// takes j = t, t + 256, .. in index order, then a tree.  V is m x 16 (zero for d >= D).  Bound by the m^2 doubles of M.
__global__ __launch_bounds__(256) void sparse_kuu_z_kernel(const double* __restrict__ Z, int m, int D, int P, SpLs ls, double sf2,
                                                           const double* __restrict__ M, int mp, const double* __restrict__ alpha,
                                                           double* __restrict__ V) {
  __shared__ double red[256 * 17];
  __shared__ double zi[GPK_MAX_D_PREDICT], ai[GPK_MAX_P];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (tid < D) zi[tid] = Z[(long long)i * D + tid] / ls.v[tid];
  if (tid >= 64 && tid - 64 < P) ai[tid - 64] = alpha[(long long)i * P + tid - 64];
  __syncthreads();
  double v[GPK_MAX_D_PREDICT];
#pragma unroll
  for (int d = 0; d < GPK_MAX_D_PREDICT; ++d) v[d] = 0.0;
  for (int j = tid; j < m; j += 256) {
    double df[GPK_MAX_D_PREDICT], d2 = 0.0;
#pragma unroll
    for (int d = 0; d < GPK_MAX_D_PREDICT; ++d) {
      df[d] = d < D ? Z[(long long)j * D + d] / ls.v[d] - zi[d] : 0.0;
      d2 = __builtin_fma(df[d], df[d], d2);
    }
    double aa = 0.0;
    for (int p = 0; p < P; ++p) aa = __builtin_fma(ai[p], alpha[(long long)j * P + p], aa);
    const double w = ((double)P * M[(long long)i * mp + j] - aa) * (sf2 * gpk_exp_neg(-0.5 * d2));     // 2 GammaK_ij Kuu0_ij
#pragma unroll
    for (int d = 0; d < GPK_MAX_D_PREDICT; ++d) v[d] = __builtin_fma(w, df[d], v[d]);
  }
#pragma unroll
  for (int d = 0; d < GPK_MAX_D_PREDICT; ++d) red[tid * 17 + d] = v[d];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off)
#pragma unroll
      for (int d = 0; d < GPK_MAX_D_PREDICT; ++d) red[tid * 17 + d] += red[(tid + off) * 17 + d];
    __syncthreads();
  }
  if (tid < GPK_MAX_D_PREDICT) V[(long long)i * GPK_MAX_D_PREDICT + tid] = red[tid];
}

// The passes over the rows behind the bound's gradient, panel by panel with the panel rule of `accumulate`.  Per panel:
// sparse_panel_kernel regenerates F = [Kfu | Yn], ONE tile GEMM Q = F Cm (rows_p x mp, k = nt: no k-slabs, a 14 336-row panel at
// m = 1024 is 896 tiles) keeps Q in registers and its epilogue reduces T = Q o Kfu, and one launch adds the tiles' sums in tile
// order to the running sums.  No floating-point atomics.
//   epilogue 4, the row pass (hyper-parameters): out = sums (17): [d] = sum_ni T_ni ((x_nd - z_id) / ls_d)^2 (d < D), [16] =
//     sum_ni T_ni; GPK_GRAD_W sums per tile, sparse_sum_kernel;
//   epilogue 5, the column pass (inducing inputs): out = R (mp x 17): [i][d] = sum_n T_ni (x_nd / ls_d - z_id / ls_d) (d < D),
//     [i][16] = sum_n T_ni; GPK_GRAD_W sums per column of every tile, sparse_colsum_kernel.
int rows_pass(gpk_handle h, int epilogue, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m, int D, int P,
              const double* ls, double sf2, const double* Cm, int64_t ldc, double* out) {
  const int64_t mp = gpk_padded(m), nt = mp + NB;
  SpLs l;
  for (int d = 0; d < D; ++d) {
    GPK_REQUIRE(h, ls[d] > 0.0 && std::isfinite(ls[d]), "sparse: length-scales must be positive");
    l.v[d] = ls[d];
  }
  const int64_t panel = sparse_panel_for(h, mp);
  const int64_t f_rows = round_up(n < panel ? n : panel, NB);
  const size_t max_tiles = (size_t)(f_rows / 64) * (size_t)(mp / 64);
  const size_t per_tile = epilogue == 4 ? (size_t)GPK_GRAD_W : (size_t)64 * GPK_GRAD_W;    // (of a 64-tile: the larger total)
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, ((size_t)f_rows * nt + max_tiles * per_tile) * sizeof(double), &ws));
  double* F = (double*)ws;
  double* partial = F + (size_t)f_rows * nt;
  gpk_time_begin(h, GPK_TIMED_SPARSE_PASS);
  for (int64_t r0 = 0; r0 < n; r0 += panel) {
    const int64_t nr = n - r0 < panel ? n - r0 : panel;
    const int64_t rows_p = round_up(nr, NB);
    hipLaunchKernelGGL(sparse_panel_kernel, dim3((unsigned)(nt / SP_TS), (unsigned)(rows_p / SP_TS)), dim3(256), 0, h->stream,
                       X + r0 * D, Yn + r0 * P, (long long)nr, Z, (int)m, D, P, l, sf2, F, (long long)nt, (int)mp);
    GPK_LAUNCH_CHECK(h);
    GemmArgs g = gemm_args(F, nt, 0, Cm, ldc, 1, partial, GPK_GRAD_W, (int)rows_p, (int)mp, (int)nt, 1.0, 0.0);
    g.epilogue = epilogue;
    g.grad_x = X + r0 * D; g.grad_z = Z; g.grad_n = (int)nr; g.grad_m = (int)m; g.grad_d = D;
    for (int d = 0; d < D; ++d) g.grad_ls[d] = ls[d];
    const int64_t tile = gpk_gemm_tile(h, g), ntiles = (rows_p / tile) * (mp / tile);
    GPK_REQUIRE(h, (size_t)ntiles * (epilogue == 4 ? 1 : (size_t)tile) <= max_tiles * (epilogue == 4 ? 1 : 64),
                "sparse: tile count of the pass over the rows");
    GPK_TRY(gpk_gemm(h, GPK_F64, g));
    if (epilogue == 4)
      hipLaunchKernelGGL(sparse_sum_kernel, dim3(GPK_GRAD_W), dim3(256), 0, h->stream, (const double*)partial, (long long)ntiles,
                         GPK_GRAD_W, out, r0 > 0 ? 1 : 0);
    else
      hipLaunchKernelGGL(sparse_colsum_kernel, dim3((unsigned)(mp * GPK_GRAD_W / 64)), dim3(256), 0, h->stream,
                         (const double*)partial, (int)(rows_p / tile), (int)(mp / tile), (int)tile, out, r0 > 0 ? 1 : 0);
    GPK_LAUNCH_CHECK(h);
  }
  gpk_time_end(h);
  return GPK_OK;
}

}  // namespace

// ---- the object behind the handle ---------------------------------------------------------------------------------
struct gpk_sparse {
  int64_t m = 0, mp = 0, nt = 0, n_rows = 0;
  int D = 0, P = 0, n_ls = 0;
  double sf2 = 1.0, noise = 0.0, jitter = 0.0, jitter_uu = 0.0, sigma2 = 0.0, bound = 0.0;
  double ls[GPK_MAX_D_PREDICT] = {0}, ls_in[GPK_MAX_D_PREDICT] = {0}, y_mean[GPK_MAX_P] = {0}, y_std[GPK_MAX_P] = {0};
  double yy_sum = 0.0;        // sum_p yy[p] of the last assembly
  int64_t held_n = 0;         // rows kept on the device by gpk_sparse_hold (0: none)
  bool finalized = false;
  // Z (m x D); S (nt x nt) the statistics; Kuu -> Luu, Wuu = Luu^-1, A1 = Wuu G, Bm = B -> LB, WB = LB^-1, WS = WB Wuu
  // (mp x mp each); winv (mp x 128); T: the scratch of gpk_trtri; pan: four (mp x 128) right-hand-side panels;
  // r, c, alpha (m x P): Wuu g / sigma^2, B^-1 r, alpha_u
  gpk_dev<double> Z, S, Kuu, Wuu, A1, Bm, WB, WS, winv, T, pan, r, c, alpha;
  // staging of gpk_sparse_update (rows) and of gpk_sparse_predict's panel path
  gpk_dev<double> rows, q;
  // gpk_sparse_hold: the held rows X (held_n x D) and their normalised targets (held_n x P); gpk_sparse_eval's gradient: the
  // coefficient matrix of the row pass ((mp + 128) x mp) and the per-row sums of sparse_dots_kernel (m x 4)
  // gradient with respect to Z: the column pass' sums (mp x 17), then the Kuu term (m x 16)
  gpk_dev<double> hX, hY, Cm, dots, zg;
  // moment matching: Q = Wuu^T Wuu - WSigma^T WSigma (mp x mp, the lower tiles), formed on first use after an assembly and
  // dropped by the next one (sparse_moment_matrix); a buffer of its own - the gradient and the path set-up reuse the others
  gpk_dev<double> Qm;
  bool q_ready = false;
  // the approximation: 0 = DTC (Titsias), 1 = FITC - the statistics are then the weighted ones, S = F^T diag(w) F, and loglam
  // is sum_i log lambda_i over the rows seen (dlog: its running value on the device, which the weighted pass adds to; the
  // host copy is read back by sparse_read_loglam).  wuu_ready: Wuu is the inverse factor at the current (Z, hyper-parameters)
  int fitc = 0;
  double loglam = 0.0;
  gpk_dev<double> dlog;
  bool wuu_ready = false;
  gpk_dev<void> work;
};

namespace {

int sparse_new(gpk_handle h, const double* Z, int64_t m, int D, int P, const double* ls, int n_ls, double sf2, double noise,
               double jitter, double jitter_uu, const double* y_mean, const double* y_std, gpk_sparse** out) {
  GPK_REQUIRE(h, Z && ls && y_mean && y_std, "sparse_begin: null pointer");
  GPK_REQUIRE(h, m >= 1 && m <= SP_MAX_M, "sparse_begin: 1 <= m <= 16384 inducing inputs");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P, "sparse_begin: need 1 <= D <= 16, 1 <= P <= GPK_MAX_P");
  GPK_REQUIRE(h, n_ls == 1 || n_ls == D, "sparse_begin: n_ls must be 1 (isotropic) or D (ARD)");
  GPK_REQUIRE(h, sf2 > 0.0 && std::isfinite(sf2) && noise >= 0.0 && jitter >= 0.0 && jitter_uu >= 0.0 &&
                     std::isfinite(noise + jitter + jitter_uu),
              "sparse_begin: sf2 must be positive, noise and the jitters non-negative");
  GPK_REQUIRE(h, noise + jitter > 0.0, "sparse_begin: the noise sigma^2 = noise + jitter must be positive");
  for (int d = 0; d < n_ls; ++d) GPK_REQUIRE(h, ls[d] > 0.0 && std::isfinite(ls[d]), "sparse_begin: length-scales must be positive");
  for (int p = 0; p < P; ++p)
    GPK_REQUIRE(h, std::isfinite(y_mean[p]) && y_std[p] > 0.0 && std::isfinite(y_std[p]), "sparse_begin: y_std must be positive");
  GPK_TRY(gpk_require_finite(h, Z, m * D, "sparse_begin", "Z"));
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  gpk_sparse_free(h);
  gpk_sparse* s = h->sparse = new gpk_sparse();
  s->m = m; s->mp = gpk_padded(m); s->nt = s->mp + NB; s->D = D; s->P = P; s->n_ls = n_ls;
  s->sf2 = sf2; s->noise = noise; s->jitter = jitter; s->jitter_uu = jitter_uu; s->sigma2 = noise + jitter;
  for (int d = 0; d < D; ++d) s->ls[d] = ls[n_ls == 1 ? 0 : d];
  for (int d = 0; d < n_ls; ++d) s->ls_in[d] = ls[d];
  for (int p = 0; p < P; ++p) { s->y_mean[p] = y_mean[p]; s->y_std[p] = y_std[p]; }
  const size_t mm = (size_t)s->mp * s->mp;
  GPK_TRY(s->Z.alloc(h, (size_t)m * D));
  GPK_TRY(s->S.alloc(h, (size_t)s->nt * s->nt));
  GPK_TRY(s->Kuu.alloc(h, mm));
  GPK_TRY(s->Wuu.alloc(h, mm));
  GPK_TRY(s->A1.alloc(h, mm));
  GPK_TRY(s->Bm.alloc(h, mm));
  GPK_TRY(s->WB.alloc(h, mm));
  GPK_TRY(s->WS.alloc(h, mm));
  GPK_TRY(s->winv.alloc(h, (size_t)s->mp * NB));
  GPK_TRY(s->T.alloc(h, gpk_trtri_work(s->mp)));
  GPK_TRY(s->pan.alloc(h, (size_t)4 * s->mp * NB));
  GPK_TRY(s->r.alloc(h, (size_t)m * P));
  GPK_TRY(s->c.alloc(h, (size_t)m * P));
  GPK_TRY(s->alpha.alloc(h, (size_t)m * P));
  GPK_CHECK_HIP(h, hipMemcpyAsync(s->Z, Z, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemsetAsync(s->S, 0, (size_t)s->nt * s->nt * sizeof(double), h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  *out = s;
  return GPK_OK;
}

// Luu Luu^T = Kuu + jitter_uu I (identity in the padding), Wuu = Luu^-1: the first step of the assembly, and under FITC what
// the weighted pass needs before the first row.  The same launches on the same (Z, hyper-parameters) wherever it is called
// from, so the finalised bits do not depend on how often it ran.
int sparse_factor_kuu(gpk_handle h, gpk_sparse* s, int* info) {
  const int64_t mp = s->mp;
  s->wuu_ready = false;
  GPK_TRY(gpk_gram(h, GPK_F64, s->Z, s->m, s->D, s->ls, s->sf2, s->jitter_uu, s->Kuu, mp));
  int rc = gpk_potrf(h, s->Kuu, mp, mp, s->winv, info);
  if (rc == GPK_NOT_PD) h->err = "sparse_finalize: Kuu + jitter_uu I is not positive definite; " + h->err;
  GPK_TRY(rc);
  GPK_TRY(gpk_trtri(h, s->Kuu, mp, mp, s->winv, s->Wuu, mp, s->T));
  s->wuu_ready = true;
  return GPK_OK;
}

// the statistics pass of the object's kind over n device rows: += F^T F (DTC) or += F^T diag(w) F and dlog += sum log lambda (FITC)
int sparse_stats(gpk_handle h, gpk_sparse* s, const double* X, const double* Yn, int64_t n) {
  if (!s->fitc) return accumulate(h, X, Yn, n, s->Z, s->m, s->D, s->P, s->ls, s->sf2, s->S, s->nt);
  if (!s->wuu_ready) {      // (an evaluation that failed in the factorisation left none)
    int info = 0;
    GPK_TRY(sparse_factor_kuu(h, s, &info));
  }
  const FitcArgs f{s->Wuu, s->mp, s->sigma2, s->dlog, nullptr};
  return accumulate(h, X, Yn, n, s->Z, s->m, s->D, s->P, s->ls, s->sf2, s->S, s->nt, &f);
}

// FITC: the running sum of log lambda_i from the device (synchronises)
int sparse_read_loglam(gpk_handle h, gpk_sparse* s) {
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  GPK_CHECK_HIP(h, hipMemcpy(&s->loglam, s->dlog, sizeof(double), hipMemcpyDeviceToHost));
  return GPK_OK;
}

// sets the kind; FITC: allocates the device sum, sets it to loglam and factors Kuu (GPK_NOT_PD with the pivot in *info)
int sparse_set_kind(gpk_handle h, gpk_sparse* s, int kind, double loglam, int* info) {
  *info = 0;
  s->finalized = false;
  s->fitc = kind;
  s->loglam = kind ? loglam : 0.0;
  if (!kind) return GPK_OK;
  if (!s->dlog) GPK_TRY(s->dlog.alloc(h, 1));
  GPK_CHECK_HIP(h, hipMemcpy(s->dlog, &s->loglam, sizeof(double), hipMemcpyHostToDevice));
  return sparse_factor_kuu(h, s, info);
}

}  // namespace

void gpk_sparse_free(gpk_handle h) {
  delete h->sparse;
  h->sparse = nullptr;
}

extern "C" int gpk_sparse_accumulate(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m,
                                     int D, int P, const double* ls, double sf2, double* S, int64_t ld) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Yn && Z && ls && S, "sparse_accumulate: null pointer");
  GPK_REQUIRE(h, n >= 1 && n < (1ll << 40) && m >= 1 && m <= SP_MAX_M, "sparse_accumulate: need n >= 1, 1 <= m <= 16384");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P, "sparse_accumulate: need 1 <= D <= 16, 1 <= P <= GPK_MAX_P");
  GPK_REQUIRE(h, ld >= gpk_padded(m) + NB && ld % 2 == 0 && ((uintptr_t)S % 16) == 0,
              "sparse_accumulate: S must be 16-byte aligned with an even ld >= gpk_padded(m) + 128");
  GPK_REQUIRE(h, sf2 > 0.0 && std::isfinite(sf2), "sparse_accumulate: sf2 must be positive");
  GPK_REQUIRE(h, h->batch == 1, "sparse_accumulate: not available in batched mode");
  return accumulate(h, X, Yn, n, Z, m, D, P, ls, sf2, S, ld);
}

extern "C" int gpk_sparse_accumulate_fitc(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m,
                                          int D, int P, const double* ls, double sf2, double* S, int64_t ld, const double* Wuu,
                                          int64_t ldw, double sigma2, double* log_lambda_sum, double* w) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Yn && Z && ls && S && Wuu && log_lambda_sum, "sparse_accumulate_fitc: null pointer");
  GPK_REQUIRE(h, n >= 1 && n < (1ll << 40) && m >= 1 && m <= SP_MAX_M, "sparse_accumulate_fitc: need n >= 1, 1 <= m <= 16384");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P,
              "sparse_accumulate_fitc: need 1 <= D <= 16, 1 <= P <= GPK_MAX_P");
  GPK_REQUIRE(h, ld >= gpk_padded(m) + NB && ld % 2 == 0 && ((uintptr_t)S % 16) == 0,
              "sparse_accumulate_fitc: S must be 16-byte aligned with an even ld >= gpk_padded(m) + 128");
  GPK_REQUIRE(h, ldw >= gpk_padded(m) && ldw % 2 == 0 && ((uintptr_t)Wuu % 16) == 0,
              "sparse_accumulate_fitc: Wuu must be 16-byte aligned with an even ldw >= gpk_padded(m)");
  GPK_REQUIRE(h, sf2 > 0.0 && std::isfinite(sf2) && sigma2 > 0.0 && std::isfinite(sigma2),
              "sparse_accumulate_fitc: sf2 and sigma2 must be positive");
  GPK_REQUIRE(h, h->batch == 1, "sparse_accumulate_fitc: not available in batched mode");
  const FitcArgs f{Wuu, ldw, sigma2, log_lambda_sum, w};
  return accumulate(h, X, Yn, n, Z, m, D, P, ls, sf2, S, ld, &f);
}

extern "C" int gpk_sparse_set_approximation(gpk_handle h, int kind, int* info) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_set_approximation: no sparse model (call gpk_sparse_begin first)");
  GPK_REQUIRE(h, info, "sparse_set_approximation: null pointer");
  GPK_REQUIRE(h, kind == GPK_SPARSE_DTC || kind == GPK_SPARSE_FITC, "sparse_set_approximation: kind must be 0 (DTC) or 1 (FITC)");
  *info = 0;
  if (kind == s->fitc) return GPK_OK;
  GPK_REQUIRE(h, s->n_rows == 0 && s->held_n == 0,
              "sparse_set_approximation: the object has seen rows - their statistics are those of the other approximation");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  return sparse_set_kind(h, s, kind, 0.0, info);
}

extern "C" int gpk_sparse_get_approximation(gpk_handle h, int* kind, double* log_lambda_sum) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_get_approximation: no sparse model");
  if (kind) *kind = s->fitc;
  if (log_lambda_sum) {
    if (s->fitc) {
      GPK_CHECK_HIP(h, hipSetDevice(h->device));
      GPK_TRY(sparse_read_loglam(h, s));
    }
    *log_lambda_sum = s->fitc ? s->loglam : 0.0;
  }
  return GPK_OK;
}

extern "C" int gpk_sparse_restore_approximation(gpk_handle h, int kind, double log_lambda_sum, int* info) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_restore_approximation: no sparse model (call gpk_sparse_import first)");
  GPK_REQUIRE(h, info, "sparse_restore_approximation: null pointer");
  GPK_REQUIRE(h, kind == GPK_SPARSE_DTC || kind == GPK_SPARSE_FITC, "sparse_restore_approximation: kind must be 0 (DTC) or 1 (FITC)");
  GPK_REQUIRE(h, std::isfinite(log_lambda_sum), "sparse_restore_approximation: the sum of log lambda must be finite");
  GPK_REQUIRE(h, s->held_n == 0, "sparse_restore_approximation: the object holds rows (their statistics are its own)");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  return sparse_set_kind(h, s, kind, log_lambda_sum, info);
}

extern "C" int gpk_sparse_begin(gpk_handle h, const double* Z, int64_t m, int D, int P, const double* ls, int n_ls, double sf2,
                                double noise, double jitter, double jitter_uu, const double* y_mean, const double* y_std) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = nullptr;
  return sparse_new(h, Z, m, D, P, ls, n_ls, sf2, noise, jitter, jitter_uu, y_mean, y_std, &s);
}

extern "C" int gpk_sparse_update(gpk_handle h, const double* X, const double* Y, int64_t n) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_update: no sparse model (call gpk_sparse_begin first)");
  GPK_REQUIRE(h, X && Y && n >= 1, "sparse_update: null pointer or no rows");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  const int D = s->D, P = s->P;
  GPK_TRY(gpk_require_finite(h, X, n * D, "sparse_update", "X"));
  GPK_TRY(gpk_require_finite(h, Y, n * P, "sparse_update", "Y"));
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  // the normalisation is the object's, fixed at gpk_sparse_begin: only then are the statistics additive
  std::vector<double> yn((size_t)n * P);
  for (int64_t i = 0; i < n; ++i)
    for (int p = 0; p < P; ++p) yn[(size_t)i * P + p] = (Y[i * P + p] - s->y_mean[p]) / s->y_std[p];
  GPK_TRY(s->rows.reserve(h, (size_t)n * (D + P) * sizeof(double)));
  double* dX = s->rows;
  double* dY = dX + (size_t)n * D;
  GPK_CHECK_HIP(h, hipMemcpyAsync(dX, X, (size_t)n * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(dY, yn.data(), (size_t)n * P * sizeof(double), hipMemcpyHostToDevice, h->stream));
  s->finalized = false;
  if (s->held_n) {      // the statistics stop being those of the held rows
    GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
    s->hX.reset();
    s->hY.reset();
    s->held_n = 0;
  }
  int rc = sparse_stats(h, s, dX, dY, n);
  if (hipStreamSynchronize(h->stream) != hipSuccess && rc == GPK_OK) {     // (yn leaves scope)
    h->err = "sparse_update: the statistics pass failed";
    rc = GPK_HIP_ERROR;
  }
  GPK_TRY(rc);
  s->n_rows += n;
  return GPK_OK;
}

namespace {

// The assembly of the model from the statistics (gpk_sparse_finalize, gpk_sparse_eval): include/gpk.h, gpk_sparse_finalize.
int sparse_assemble(gpk_handle h, gpk_sparse* s, int* info) {
  const int64_t mp = s->mp;
  const int imp = (int)mp, P = s->P;
  const double is2 = 1.0 / s->sigma2;
  *info = 0;
  s->finalized = false;
  s->q_ready = false;      // (Q belongs to the factors this assembly overwrites)
  GPK_TRY(sparse_factor_kuu(h, s, info));
  int rc;
  // A1 = Wuu G (Wuu lower: k < row-tile end), B = I + A1 Wuu^T / sigma^2 (k < column-tile end; every tile, so that the
  // factorisation finds whole diagonal tiles).  G is zero in the padding, so B is the identity there.
  {
    GemmArgs g = gemm_args(s->Wuu, mp, 0, s->S, s->nt, 1, s->A1, mp, imp, imp, imp, 1.0, 0.0);
    g.ke0 = NB; g.ke_row = NB; g.heavy_first = 1;
    GPK_TRY(gpk_gemm(h, GPK_F64, g));
  }
  {
    GemmArgs g = gemm_args(s->A1, mp, 0, s->Wuu, mp, 0, s->Bm, mp, imp, imp, imp, is2, 0.0);
    g.ke0 = NB; g.ke_col = NB;
    GPK_TRY(gpk_gemm(h, GPK_F64, g));
  }
  double* d_out = h->d_small + 400;     // [tr(B) - mp, yy[0 .. P)]: free doubles of the pinned block (gpk_internal.h)
  hipLaunchKernelGGL(sparse_diag_kernel, dim3(1), dim3(256), 0, h->stream, s->Bm, (long long)mp, imp, s->S, (long long)s->nt,
                     P, d_out);
  GPK_LAUNCH_CHECK(h);
  rc = gpk_potrf(h, s->Bm, mp, mp, s->winv, info);      // LB LB^T = B
  if (rc == GPK_NOT_PD) h->err = "sparse_finalize: B = I + Wuu G Wuu^T / sigma^2 is not positive definite; " + h->err;
  GPK_TRY(rc);
  const double tr_a = h->h_small[400];
  double yy[GPK_MAX_P];
  for (int p = 0; p < P; ++p) yy[p] = h->h_small[401 + p];
  GPK_TRY(gpk_trtri(h, s->Bm, mp, mp, s->winv, s->WB, mp, s->T));
  // WSigma = LB^-1 Wuu: lower tiles (column-tile start <= k < row-tile end) of a zeroed matrix - the inverse-factor layout
  // of gpk_predict_var_inv (lower tiles, zeros right of the diagonal)
  GPK_CHECK_HIP(h, hipMemsetAsync(s->WS, 0, (size_t)mp * mp * sizeof(double), h->stream));
  {
    GemmArgs g = gemm_args(s->WB, mp, 0, s->Wuu, mp, 1, s->WS, mp, imp, imp, imp, 1.0, 0.0);
    g.kb_col = NB; g.ke0 = NB; g.ke_row = NB; g.lower_only = 1;
    GPK_TRY(gpk_gemm(h, GPK_F64, g));
  }
  // r = Wuu g / sigma^2, c = B^-1 r = WB^T (WB r), alpha_u = Wuu^T c: four products on 128-column panels (the targets'
  // columns of S are g, zero beyond P)
  double *Rp = s->pan, *Cz = Rp + (size_t)mp * NB, *Cp = Cz + (size_t)mp * NB, *Ap = Cp + (size_t)mp * NB;
  {
    GemmArgs g = gemm_args(s->Wuu, mp, 0, s->S + mp, s->nt, 1, Rp, NB, imp, NB, imp, is2, 0.0);
    g.ke0 = NB; g.ke_row = NB; g.heavy_first = 1;
    GPK_TRY(gpk_gemm(h, GPK_F64, g));
    GemmArgs g2 = gemm_args(s->WB, mp, 0, Rp, NB, 1, Cz, NB, imp, NB, imp, 1.0, 0.0);
    g2.ke0 = NB; g2.ke_row = NB; g2.heavy_first = 1;
    GPK_TRY(gpk_gemm(h, GPK_F64, g2));
    GemmArgs g3 = gemm_args(s->WB, mp, 1, Cz, NB, 1, Cp, NB, imp, NB, imp, 1.0, 0.0);
    g3.kb_row = NB;
    GPK_TRY(gpk_gemm(h, GPK_F64, g3));
    GemmArgs g4 = gemm_args(s->Wuu, mp, 1, Cp, NB, 1, Ap, NB, imp, NB, imp, 1.0, 0.0);
    g4.kb_row = NB;
    GPK_TRY(gpk_gemm(h, GPK_F64, g4));
  }
  const long long tot = (long long)s->m * P;
  hipLaunchKernelGGL(sparse_unpack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, Rp, Cp, Ap,
                     (long long)s->m, P, s->r, s->c, s->alpha);
  GPK_LAUNCH_CHECK(h);
  // terms[0] = sum log diag LB, terms[1 + p] = r_p^T B^-1 r_p (synchronises)
  double terms[1 + GPK_MAX_P];
  GPK_TRY(gpk_lml_terms(h, s->Bm, s->m, mp, s->r, s->c, P, terms));
  const double N = (double)s->n_rows, s2 = s->sigma2;
  double bound = 0.0;
  if (s->fitc) {
    // log N(y | 0, Qff + diag(lambda)): -N/2 log sigma^2 becomes -1/2 sum log lambda_i, no trace term; yy and r carry the weights
    GPK_TRY(sparse_read_loglam(h, s));
    for (int p = 0; p < P; ++p)
      bound += -0.5 * N * std::log(2.0 * M_PI) - 0.5 * s->loglam - terms[0] - 0.5 * yy[p] / s2 + 0.5 * terms[1 + p];
  } else {
    for (int p = 0; p < P; ++p)
      bound += -0.5 * N * std::log(2.0 * M_PI * s2) - terms[0] - 0.5 * (N * s->sf2 - s2 * tr_a) / s2 - 0.5 * yy[p] / s2 +
               0.5 * terms[1 + p];
  }
  s->bound = bound;
  s->yy_sum = 0.0;
  for (int p = 0; p < P; ++p) s->yy_sum += yy[p];
  s->finalized = true;
  return GPK_OK;
}

// The gradient of the bound of the model just assembled, with respect to log [ls_0 .. ls_{D-1}, noise, sf2] (g: D + 2 values).
// Buffers of the assembly that the served model does not need are reused: Kuu (Luu) <- Kuu^-1, Bm (LB) <- Sigma~, WB <-
// Kuu^-1 G, A1 <- Kuu^-1 G Kuu^-1 and then the matrix of the Kuu term, pan[1] <- G alpha_u.  One synchronisation.
// gradZ != NULL (host m x D): also dL/dZ in raw coordinates, (U + V) / ls - behind the launches above, the matrix of the Kuu
// term is mirrored to a full matrix, sparse_kuu_z_kernel forms V and the column pass U (include/gpk.h, gpk_sparse_eval_z).
int sparse_gradient(gpk_handle h, gpk_sparse* s, double* g, double* gradZ) {
  const int64_t m = s->m, mp = s->mp, nt = s->nt;
  const int imp = (int)mp, P = s->P, D = s->D;
  const double s2 = s->sigma2, is2 = 1.0 / s2;
  if (!s->Cm) GPK_TRY(s->Cm.alloc(h, (size_t)nt * mp));
  if (!s->dots) GPK_TRY(s->dots.alloc(h, (size_t)m * 4));
  double *Ki = s->Kuu, *Si = s->Bm, *H = s->WB, *M3 = s->A1;
  double *Ap = s->pan + (size_t)3 * mp * NB, *GA = s->pan + (size_t)mp * NB;
  const unsigned nb32 = (unsigned)(mp / 32), mirror_blocks = nb32 * (nb32 + 1) / 2;
  // Kuu^-1 = Wuu^T Wuu and Sigma~ = WSigma^T WSigma: the lower tiles, mirrored to full matrices
  GPK_TRY(gpk_wtw(h, s->Wuu, mp, mp, Ki, mp));
  hipLaunchKernelGGL(sparse_reduce_kernel, dim3(mirror_blocks), dim3(256), 0, h->stream, Ki, (long long)mp, (const double*)Ki, 0,
                     0ll, imp);
  GPK_LAUNCH_CHECK(h);
  // H = Kuu^-1 G = Wuu^T A1 (Wuu lower: k >= row-tile start)
  {
    GemmArgs a = gemm_args(s->Wuu, mp, 1, s->A1, mp, 1, H, mp, imp, imp, imp, 1.0, 0.0);
    a.kb_row = NB;
    GPK_TRY(gpk_gemm(h, GPK_F64, a));
  }
  GPK_TRY(gpk_wtw(h, s->WS, mp, mp, Si, mp));
  hipLaunchKernelGGL(sparse_reduce_kernel, dim3(mirror_blocks), dim3(256), 0, h->stream, Si, (long long)mp, (const double*)Si, 0,
                     0ll, imp);
  GPK_LAUNCH_CHECK(h);
  // M3 = H Kuu^-1: the lower tiles
  {
    GemmArgs a = gemm_args(H, mp, 0, Ki, mp, 0, M3, mp, imp, imp, imp, 1.0, 0.0);
    a.lower_only = 1;
    GPK_TRY(gpk_gemm(h, GPK_F64, a));
  }
  {
    const long long tot = (long long)nt * mp;
    hipLaunchKernelGGL(sparse_coef_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, (const double*)Ki,
                       (const double*)Si, M3, (const double*)s->alpha, (int)m, imp, P, is2, s->Cm.p);
    GPK_LAUNCH_CHECK(h);
  }
  // G alpha_u on the 128-column panel of alpha_u (zero beyond P and m)
  {
    GemmArgs a = gemm_args(s->S, nt, 0, Ap, NB, 1, GA, NB, imp, NB, imp, 1.0, 0.0);
    GPK_TRY(gpk_gemm(h, GPK_F64, a));
  }
  double *d_kuu = h->d_small + 64, *d_rows = h->d_small + 96, *d_dots = h->d_small + 128;   // free doubles of the pinned block
  hipLaunchKernelGGL(sparse_dots_kernel, dim3((unsigned)m), dim3(256), 0, h->stream, (const double*)Ki, (const double*)Si,
                     (const double*)s->S, (long long)nt, (const double*)s->alpha, (const double*)GA, (int)m, imp, P, s->dots.p);
  GPK_LAUNCH_CHECK(h);
  hipLaunchKernelGGL(sparse_sum_kernel, dim3(4), dim3(256), 0, h->stream, (const double*)s->dots, (long long)m, 4, d_dots, 0);
  GPK_LAUNCH_CHECK(h);
  // the Kuu term: gpk_lml_grad's sums on (Z, alpha_u, Kuu^-1 - Sigma~ - M3 / s2) are -2 sum GammaK o Kuu0 o (...)
  GPK_TRY(gpk_lml_grad_enqueue(h, s->Z, m, D, s->ls, s->sf2, s->alpha, P, M3, mp, d_kuu));
  GPK_TRY(rows_pass(h, 4, s->hX, s->hY, s->held_n, s->Z, m, D, P, s->ls, s->sf2, s->Cm, mp, d_rows));
  std::vector<double> zg;
  if (gradZ) {
    const size_t nr = (size_t)mp * GPK_GRAD_W, nv = (size_t)m * GPK_MAX_D_PREDICT;
    if (!s->zg) GPK_TRY(s->zg.alloc(h, nr + nv));
    double *R = s->zg, *V = R + nr;
    SpLs l;
    for (int d = 0; d < D; ++d) l.v[d] = s->ls[d];
    hipLaunchKernelGGL(sparse_reduce_kernel, dim3(mirror_blocks), dim3(256), 0, h->stream, M3, (long long)mp, (const double*)M3, 0,
                       0ll, imp);
    GPK_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(sparse_kuu_z_kernel, dim3((unsigned)m), dim3(256), 0, h->stream, (const double*)s->Z, (int)m, D, P, l, s->sf2,
                       (const double*)M3, imp, (const double*)s->alpha, V);
    GPK_LAUNCH_CHECK(h);
    GPK_TRY(rows_pass(h, 5, s->hX, s->hY, s->held_n, s->Z, m, D, P, s->ls, s->sf2, s->Cm, mp, R));
    zg.resize(nr + nv);      // (pageable: the runtime stages this copy; the small sums above come through the pinned block)
    GPK_CHECK_HIP(h, hipMemcpyAsync(zg.data(), R, (nr + nv) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  if (gradZ)
    for (int64_t i = 0; i < m; ++i)
      for (int d = 0; d < D; ++d)
        gradZ[i * D + d] = (zg[(size_t)i * GPK_GRAD_W + d] + zg[(size_t)mp * GPK_GRAD_W + (size_t)i * GPK_MAX_D_PREDICT + d]) / s->ls[d];
  const double *kuu = h->h_small + 64, *rows = h->h_small + 96, *dots = h->h_small + 128;
  const double N = (double)s->n_rows, Pd = (double)P, sf2 = s->sf2;
  for (int d = 0; d < D; ++d) g[d] = rows[d] - 0.5 * kuu[d];
  g[D] = s->noise * (Pd * (-N / (2.0 * s2) + N * sf2 / (2.0 * s2 * s2) - dots[0] / (2.0 * s2 * s2) + dots[1] / (2.0 * s2 * s2)) +
                     s->yy_sum / (2.0 * s2 * s2) - dots[2] / (s2 * s2) + dots[3] / (2.0 * s2 * s2));
  g[D + 1] = rows[16] - 0.5 * kuu[17] - Pd * N * sf2 / (2.0 * s2);
  return GPK_OK;
}

}  // namespace

extern "C" int gpk_sparse_finalize(gpk_handle h, int* info) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_finalize: no sparse model (call gpk_sparse_begin first)");
  GPK_REQUIRE(h, info, "sparse_finalize: null pointer");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  return sparse_assemble(h, s, info);
}

extern "C" int gpk_sparse_grad_pass(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m, int D,
                                    int P, const double* ls, double sf2, const double* Cm, int64_t ldc, double* sums) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Yn && Z && ls && Cm && sums, "sparse_grad_pass: null pointer");
  GPK_REQUIRE(h, n >= 1 && n < (1ll << 40) && m >= 1 && m <= SP_MAX_M, "sparse_grad_pass: need n >= 1, 1 <= m <= 16384");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P, "sparse_grad_pass: need 1 <= D <= 16, 1 <= P <= GPK_MAX_P");
  GPK_REQUIRE(h, ldc >= gpk_padded(m) && ldc % 2 == 0 && ((uintptr_t)Cm % 16) == 0,
              "sparse_grad_pass: Cm must be 16-byte aligned with an even ldc >= gpk_padded(m)");
  GPK_REQUIRE(h, sf2 > 0.0 && std::isfinite(sf2), "sparse_grad_pass: sf2 must be positive");
  GPK_REQUIRE(h, h->batch == 1, "sparse_grad_pass: not available in batched mode");
  return rows_pass(h, 4, X, Yn, n, Z, m, D, P, ls, sf2, Cm, ldc, sums);
}

extern "C" int gpk_sparse_zgrad_pass(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m, int D,
                                     int P, const double* ls, double sf2, const double* Cm, int64_t ldc, double* R) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Yn && Z && ls && Cm && R, "sparse_zgrad_pass: null pointer");
  GPK_REQUIRE(h, n >= 1 && n < (1ll << 40) && m >= 1 && m <= SP_MAX_M, "sparse_zgrad_pass: need n >= 1, 1 <= m <= 16384");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P, "sparse_zgrad_pass: need 1 <= D <= 16, 1 <= P <= GPK_MAX_P");
  GPK_REQUIRE(h, ldc >= gpk_padded(m) && ldc % 2 == 0 && ((uintptr_t)Cm % 16) == 0,
              "sparse_zgrad_pass: Cm must be 16-byte aligned with an even ldc >= gpk_padded(m)");
  GPK_REQUIRE(h, sf2 > 0.0 && std::isfinite(sf2), "sparse_zgrad_pass: sf2 must be positive");
  GPK_REQUIRE(h, h->batch == 1, "sparse_zgrad_pass: not available in batched mode");
  return rows_pass(h, 5, X, Yn, n, Z, m, D, P, ls, sf2, Cm, ldc, R);
}

extern "C" int gpk_sparse_hold(gpk_handle h, const double* X, const double* Y, int64_t n) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_hold: no sparse model (call gpk_sparse_begin first)");
  GPK_REQUIRE(h, n >= 0 && (n == 0 || (X && Y)), "sparse_hold: null pointer or negative row count");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = s->D, P = s->P;
  if (n > 0) {
    GPK_TRY(gpk_require_finite(h, X, n * D, "sparse_hold", "X"));
    GPK_TRY(gpk_require_finite(h, Y, n * P, "sparse_hold", "Y"));
  }
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  s->hX.reset();
  s->hY.reset();
  s->held_n = 0;
  if (n == 0) return GPK_OK;
  std::vector<double> yn((size_t)n * P);
  for (int64_t i = 0; i < n; ++i)
    for (int p = 0; p < P; ++p) yn[(size_t)i * P + p] = (Y[i * P + p] - s->y_mean[p]) / s->y_std[p];
  GPK_TRY(s->hX.alloc(h, (size_t)n * D));
  GPK_TRY(s->hY.alloc(h, (size_t)n * P));
  GPK_CHECK_HIP(h, hipMemcpyAsync(s->hX, X, (size_t)n * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(s->hY, yn.data(), (size_t)n * P * sizeof(double), hipMemcpyHostToDevice, h->stream));
  // the statistics become those of these rows
  s->finalized = false;
  s->n_rows = 0;
  GPK_CHECK_HIP(h, hipMemsetAsync(s->S, 0, (size_t)s->nt * s->nt * sizeof(double), h->stream));
  if (s->fitc) GPK_CHECK_HIP(h, hipMemsetAsync(s->dlog, 0, sizeof(double), h->stream));
  int rc = sparse_stats(h, s, s->hX, s->hY, n);
  if (hipStreamSynchronize(h->stream) != hipSuccess && rc == GPK_OK) {     // (yn leaves scope)
    h->err = "sparse_hold: the statistics pass failed";
    rc = GPK_HIP_ERROR;
  }
  GPK_TRY(rc);
  s->n_rows = n;
  s->held_n = n;
  return GPK_OK;
}

namespace {

// gpk_sparse_eval (Z == NULL, gradZ == NULL: its launches) and gpk_sparse_eval_z
int sparse_eval(gpk_handle h, const double* Z, const double* ls, int n_ls, double sf2, double noise, double* bound, double* grad,
                double* gradZ, int* info) {
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_eval: no sparse model (call gpk_sparse_begin first)");
  GPK_REQUIRE(h, s->held_n > 0, "sparse_eval: no held rows (call gpk_sparse_hold; gpk_sparse_update releases them)");
  GPK_REQUIRE(h, ls && bound && info, "sparse_eval: null pointer");
  GPK_REQUIRE(h, n_ls == s->n_ls, "sparse_eval: n_ls must be that of gpk_sparse_begin");
  GPK_REQUIRE(h, sf2 > 0.0 && std::isfinite(sf2) && noise >= 0.0 && std::isfinite(noise) && noise + s->jitter > 0.0,
              "sparse_eval: sf2 and the noise sigma^2 = noise + jitter must be positive");
  for (int d = 0; d < n_ls; ++d) GPK_REQUIRE(h, ls[d] > 0.0 && std::isfinite(ls[d]), "sparse_eval: length-scales must be positive");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_REQUIRE(h, !(s->fitc && (grad || gradZ)),
              "sparse_eval: the gradient of the FITC likelihood is not available (the object's approximation is FITC: pass grad = "
              "gradZ = NULL, or train as DTC)");
  if (Z) GPK_TRY(gpk_require_finite(h, Z, s->m * s->D, "sparse_eval", "Z"));
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = s->D;
  *info = 0;
  s->finalized = false;
  if (Z) {      // (the caller's array is read before the call goes on: no return path leaves the copy in flight)
    GPK_CHECK_HIP(h, hipMemcpyAsync(s->Z, Z, (size_t)s->m * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  }
  s->sf2 = sf2; s->noise = noise; s->sigma2 = noise + s->jitter;
  for (int d = 0; d < D; ++d) s->ls[d] = ls[n_ls == 1 ? 0 : d];
  for (int d = 0; d < n_ls; ++d) s->ls_in[d] = ls[d];
  s->wuu_ready = false;
  if (s->fitc) {      // the weights need the inverse factor at these hyper-parameters (and this Z) before the first row
    GPK_TRY(sparse_factor_kuu(h, s, info));
    GPK_CHECK_HIP(h, hipMemsetAsync(s->dlog, 0, sizeof(double), h->stream));
  }
  // the statistics of the held rows at these hyper-parameters
  GPK_CHECK_HIP(h, hipMemsetAsync(s->S, 0, (size_t)s->nt * s->nt * sizeof(double), h->stream));
  gpk_time_begin(h, GPK_TIMED_SPARSE_STATS);
  int rc = sparse_stats(h, s, s->hX, s->hY, s->held_n);
  gpk_time_end(h);
  GPK_TRY(rc);
  s->n_rows = s->held_n;
  GPK_TRY(sparse_assemble(h, s, info));
  *bound = s->bound;
  if (!grad && !gradZ) return GPK_OK;
  double g[GPK_MAX_D_PREDICT + 2];
  rc = sparse_gradient(h, s, g, gradZ);
  if (rc != GPK_OK) { s->finalized = false; return rc; }
  if (!grad) return GPK_OK;
  if (n_ls == 1) {
    double t = 0.0;
    for (int d = 0; d < D; ++d) t += g[d];
    grad[0] = t;
  } else {
    for (int d = 0; d < D; ++d) grad[d] = g[d];
  }
  grad[n_ls] = g[D];
  grad[n_ls + 1] = g[D + 1];
  return GPK_OK;
}

}  // namespace

extern "C" int gpk_sparse_eval(gpk_handle h, const double* ls, int n_ls, double sf2, double noise, double* bound, double* grad,
                               int* info) {
  if (!h) return GPK_BAD_ARG;
  return sparse_eval(h, nullptr, ls, n_ls, sf2, noise, bound, grad, nullptr, info);
}

extern "C" int gpk_sparse_eval_z(gpk_handle h, const double* Z, const double* ls, int n_ls, double sf2, double noise, double* bound,
                                 double* grad, double* gradZ, int* info) {
  if (!h) return GPK_BAD_ARG;
  return sparse_eval(h, Z, ls, n_ls, sf2, noise, bound, grad, gradZ, info);
}

// Greedy conditional-variance selection (gpk_select.hip) under the object's kernel: host rows, or the held ones.  Everything
// the call allocates is a local gpk_dev: every return frees it, and the object is only read.
extern "C" int gpk_sparse_select(gpk_handle h, const double* X, int64_t n, int64_t m_max, double min_var, double tol, int64_t* idx,
                                 double* trace, double* dmax, int64_t* selected) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_select: no sparse model (call gpk_sparse_begin first)");
  GPK_REQUIRE(h, idx && trace && dmax && selected, "sparse_select: null pointer");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  if (!X) {
    GPK_REQUIRE(h, s->held_n > 0, "sparse_select: no held rows (call gpk_sparse_hold; gpk_sparse_update releases them)");
    GPK_REQUIRE(h, n == s->held_n, "sparse_select: n must be the number of held rows");
  }
  GPK_REQUIRE(h, n >= 1 && m_max >= 1 && m_max <= n && m_max <= SP_MAX_M, "sparse_select: need 1 <= m_max <= min(n, 16384)");
  GPK_REQUIRE(h, min_var >= 0.0 && tol >= 0.0 && std::isfinite(min_var) && std::isfinite(tol),
              "sparse_select: min_var and tol must be non-negative");
  const int D = s->D;
  if (X) GPK_TRY(gpk_require_finite(h, X, n * D, "sparse_select", "X"));
  const size_t bytes = gpk_greedy_select_bytes(n, m_max);
  GPK_REQUIRE(h, bytes > 0, "sparse_select: n too large");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  gpk_dev<double> work, rows, out;
  gpk_dev<int64_t> iout;
  GPK_TRY(work.alloc(h, bytes / sizeof(double)));
  GPK_TRY(out.alloc(h, (size_t)2 * m_max));
  GPK_TRY(iout.alloc(h, (size_t)m_max + 1));
  const double* dX = s->hX;
  if (X) {
    GPK_TRY(rows.alloc(h, (size_t)n * D));
    GPK_CHECK_HIP(h, hipMemcpyAsync(rows, X, (size_t)n * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    dX = rows;
  }
  int rc = gpk_greedy_select(h, dX, n, D, s->ls, D, s->sf2, m_max, min_var, tol, work, iout, out, out + m_max, iout + m_max);
  // (the launches read the local buffers: drain the stream on every path before they are freed)
  std::vector<int64_t> hi((size_t)m_max + 1);
  std::vector<double> ho((size_t)2 * m_max);
  if (rc == GPK_OK && (hipMemcpyAsync(hi.data(), iout, hi.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                       hipMemcpyAsync(ho.data(), out, ho.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess)) {
    h->err = "sparse_select: copying the result failed";
    rc = GPK_HIP_ERROR;
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess && rc == GPK_OK) {
    h->err = "sparse_select: the selection failed";
    rc = GPK_HIP_ERROR;
  }
  GPK_TRY(rc);
  const int64_t sel = hi[(size_t)m_max];
  GPK_REQUIRE(h, sel >= 0 && sel <= m_max, "sparse_select: the selection returned an impossible count");
  for (int64_t t = 0; t < sel; ++t) { idx[t] = hi[(size_t)t]; trace[t] = ho[(size_t)t]; dmax[t] = ho[(size_t)(m_max + t)]; }
  *selected = sel;
  return GPK_OK;
}

extern "C" int gpk_sparse_bound(gpk_handle h, double* bound, int64_t* n_rows) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, "sparse_bound: no finalised sparse model (call gpk_sparse_finalize first)");
  if (bound) *bound = s->bound;
  if (n_rows) *n_rows = s->n_rows;
  return GPK_OK;
}

namespace {

// The one place that takes sparse models apart for the serving routines (gpk_serve.hip): one model with its P outputs, or B
// single-output models of equal m and D, as the two-factor description - the inducing inputs as the training inputs, alpha_u,
// W[0] = Wuu, W[1] = WSigma.  The description points into this object.
struct SparseServe {
  int B = 0, D = 0, P = 0;
  int64_t m = 0, mp = 0;
  gpk_sparse* s[GPK_SMALL_MAX_MODELS] = {nullptr};
  const double *Z[GPK_SMALL_MAX_MODELS], *alpha[GPK_SMALL_MAX_MODELS], *W0[GPK_SMALL_MAX_MODELS], *W1[GPK_SMALL_MAX_MODELS];
  double ls[GPK_SMALL_MAX_MODELS * GPK_MAX_D_PREDICT], sf2[GPK_SMALL_MAX_MODELS], kss[GPK_SMALL_MAX_MODELS],
      noise[GPK_SMALL_MAX_MODELS], y_mean[GPK_MAX_P], y_std[GPK_MAX_P], floor_ = 0.0;
  static_assert(GPK_SMALL_MAX_MODELS <= GPK_MAX_P, "y_mean / y_std: P outputs of one model, or one of each of B models");

  void fill(int B_, gpk_sparse* const* models, int var_includes_noise) {
    B = B_; D = models[0]->D; P = models[0]->P; m = models[0]->m; mp = models[0]->mp;
    floor_ = gpk_var_floor(var_includes_noise);
    for (int b = 0; b < B; ++b) {
      gpk_sparse* sp = s[b] = models[b];
      Z[b] = sp->Z; alpha[b] = sp->alpha; W0[b] = sp->Wuu; W1[b] = sp->WS;
      for (int d = 0; d < D; ++d) ls[b * D + d] = sp->ls[d];
      sf2[b] = sp->sf2; noise[b] = sp->noise; kss[b] = gpk_kss(sp->sf2, sp->noise, var_includes_noise);
      for (int p = 0; p < P; ++p) { y_mean[b * P + p] = sp->y_mean[p]; y_std[b * P + p] = sp->y_std[p]; }
    }
  }
  ServeModels models() const { return {B, P, 2, Z, alpha, m, D, ls, sf2, y_mean, y_std, {W0, W1}, mp, mp, kss, floor_, noise}; }
  // up to 32 queries: the two-factor small-batch kernels (gpk_small.hip) - one K* per model, the two inverse factors combined on
  // the device, the launch counts of one single-output model, one synchronisation
  bool small(gpk_handle h, int64_t M) const { return h->small_path && M <= GPK_SMALL_MAX_M && gpk_small_ok(mp, D, P, M); }
  // The small route's dvar (B, M, D), and cov (B, M, M) of either route, come in normalised-target units: output p of model b
  // carries y_std[b * P + p]^2, as in gpk_predict_model_grad / gpk_predict_model_cov.  dvar (B, M, P, D); cov (B, P, M, M);
  // P == 1: in place if the caller likes.
  void scale_dvar(const double* g, int64_t M, double* dvar) const {
    for (int64_t i = 0; i < B * M; ++i)
      for (int p = 0; p < P; ++p) {
        const double s2 = y_std[i / M * P + p] * y_std[i / M * P + p];
        for (int d = 0; d < D; ++d) dvar[(i * P + p) * D + d] = g[i * D + d] * s2;
      }
  }
  void scale_cov(const double* sig, int64_t M, double* cov) const {
    const size_t nc = (size_t)M * M;
    for (int o = 0; o < B * P; ++o) {
      const double s2 = y_std[o] * y_std[o];
      for (size_t i = 0; i < nc; ++i) cov[o * nc + i] = sig[o / P * nc + i] * s2;
    }
  }
};

}  // namespace

// The serving bodies take the object apart from the handle: h supplies the stream, the pinned staging block and the work area,
// s the model and its own panel staging (the single entries: s = h->sparse; the batch entries: one model of the list).
static int sparse_predict(gpk_handle h, gpk_sparse* s, const double* Xq, int64_t M, double* mean, double* var,
                          int var_includes_noise) {
  GPK_REQUIRE(h, Xq && mean && M >= 1, "sparse_predict: null pointer or empty batch");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = s->D, P = s->P;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "sparse_predict", "Xq"));
  const double kss = gpk_kss(s->sf2, s->noise, var_includes_noise), floor_ = gpk_var_floor(var_includes_noise);
  const double none = -std::numeric_limits<double>::max();
  const int64_t m = s->m, mp = s->mp;
  SparseServe sv;
  sv.fill(1, &s, var_includes_noise);
  if (sv.small(h, M)) return gpk_serve_predict(h, sv.models(), true, Xq, M, mean, var);      // the mean one launch, mean + variance two
  // query panels: the fused mean and two variance launches (one per inverse factor), combined on the device
  const int64_t panel = gpk_panel_rows(GPK_HOST_MAX_M, 1, M);      // (no byte budget: at most GPK_HOST_MAX_M rows)
  const size_t nq = (size_t)panel * D, nm = (size_t)panel * P;
  GPK_TRY(s->q.reserve(h, (nq + nm + (var ? 2 * (size_t)panel + nm : 0)) * sizeof(double)));
  if (var) GPK_TRY(s->work.reserve(h, (size_t)mp * panel * sizeof(double)));
  double *dq = s->q, *dmean = dq + nq, *dv0 = dmean + nm, *dv1 = dv0 + panel, *dvar = dv1 + panel;
  SpP ys;
  for (int p = 0; p < GPK_MAX_P; ++p) ys.v[p] = p < P ? s->y_std[p] : 1.0;
  return gpk_query_panels(h, Xq, M, D * sizeof(double), panel, dq, [&](int64_t m0, int64_t mc) -> int {
    GPK_TRY(gpk_predict_mean(h, GPK_F64, s->Z, s->alpha, m, D, P, s->ls, s->sf2, s->y_mean, s->y_std, dq, mc, dmean));
    GPK_CHECK_HIP(h, hipMemcpyAsync(mean + m0 * P, dmean, (size_t)mc * P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (var) {
      GPK_TRY(gpk_predict_var_inv(h, GPK_F64, s->Z, m, D, s->ls, s->sf2, s->Wuu, mp, mp, dq, mc, kss, none, s->work, dv0));
      GPK_TRY(gpk_predict_var_inv(h, GPK_F64, s->Z, m, D, s->ls, s->sf2, s->WS, mp, mp, dq, mc, 0.0, none, s->work, dv1));
      const long long tot = (long long)mc * P;
      hipLaunchKernelGGL(sparse_var_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, dv0, dv1,
                         (long long)mc, P, ys, floor_, dvar);
      GPK_LAUNCH_CHECK(h);
      GPK_CHECK_HIP(h, hipMemcpyAsync(var + m0 * P, dvar, (size_t)mc * P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    return GPK_OK;
  });
}

extern "C" int gpk_sparse_predict(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var,
                                  int var_includes_noise) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, "sparse_predict: no finalised sparse model (call gpk_sparse_finalize first)");
  return sparse_predict(h, s, Xq, M, mean, var, var_includes_noise);
}

static int sparse_predict_grad(gpk_handle h, gpk_sparse* s, const double* Xq, int64_t M, double* mean, double* var, double* dmean,
                               double* dvar, int var_includes_noise) {
  GPK_REQUIRE(h, Xq && mean && dmean && M >= 1, "sparse_predict_grad: null pointer or empty batch");
  GPK_REQUIRE(h, (var == nullptr) == (dvar == nullptr), "sparse_predict_grad: var and dvar come together (both or neither)");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = s->D, P = s->P;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "sparse_predict_grad", "Xq"));
  const double kss = gpk_kss(s->sf2, s->noise, var_includes_noise), floor_ = gpk_var_floor(var_includes_noise);
  const double none = -std::numeric_limits<double>::max();
  const int64_t m = s->m, mp = s->mp;
  SparseServe sv;
  sv.fill(1, &s, var_includes_noise);
  if (sv.small(h, M)) {      // mean + Jacobian one launch, all four results three
    std::vector<double> g1(var ? (size_t)M * D : 0);
    GPK_TRY(gpk_serve_grad(h, sv.models(), true, Xq, M, mean, var, dmean, var ? g1.data() : nullptr));
    if (var) sv.scale_dvar(g1.data(), M, dvar);
    return GPK_OK;
  }
  // query panels: the fused mean and its Jacobian, the variance gradient once per inverse factor (three mp x panel work panels
  // within 6 GiB, as gpk_predict_host_grad keeps them), combined on the device
  const int64_t panel = gpk_panel_rows(6ull << 30, (size_t)3 * mp * sizeof(double), M);
  const size_t nq = (size_t)panel * D, nm = (size_t)panel * P, nj = nm * D;
  GPK_TRY(s->q.reserve(h, (nq + nm + nj + (var ? 2 * (size_t)panel + 2 * nq + nm + nj : 0)) * sizeof(double)));
  if (var) GPK_TRY(s->work.reserve(h, (size_t)3 * mp * panel * sizeof(double)));
  double *dq = s->q, *dmn = dq + nq, *ddm = dmn + nm, *dv0 = ddm + nj, *dv1 = dv0 + panel, *dg0 = dv1 + panel, *dg1 = dg0 + nq,
         *dvar_ = dg1 + nq, *ddv = dvar_ + nm;
  SpP ys;
  for (int p = 0; p < GPK_MAX_P; ++p) ys.v[p] = p < P ? s->y_std[p] : 1.0;
  return gpk_query_panels(h, Xq, M, D * sizeof(double), panel, dq, [&](int64_t m0, int64_t mc) -> int {
    GPK_TRY(gpk_predict_mean(h, GPK_F64, s->Z, s->alpha, m, D, P, s->ls, s->sf2, s->y_mean, s->y_std, dq, mc, dmn));
    GPK_TRY(gpk_predict_mean_grad(h, s->Z, s->alpha, m, D, P, s->ls, s->sf2, s->y_std, dq, mc, ddm));
    GPK_CHECK_HIP(h, hipMemcpyAsync(mean + m0 * P, dmn, (size_t)mc * P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_CHECK_HIP(h, hipMemcpyAsync(dmean + m0 * P * D, ddm, (size_t)mc * P * D * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (var) {
      GPK_TRY(gpk_predict_var_grad_inv(h, s->Z, m, D, s->ls, s->sf2, s->Wuu, mp, mp, dq, mc, kss, none, (double*)s->work.p, dv0, dg0));
      GPK_TRY(gpk_predict_var_grad_inv(h, s->Z, m, D, s->ls, s->sf2, s->WS, mp, mp, dq, mc, 0.0, none, (double*)s->work.p, dv1, dg1));
      const long long tot = (long long)mc * P * D;
      hipLaunchKernelGGL(sparse_var_grad_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, dv0, dv1, dg0, dg1,
                         (long long)mc, P, D, ys, floor_, dvar_, ddv);
      GPK_LAUNCH_CHECK(h);
      GPK_CHECK_HIP(h, hipMemcpyAsync(var + m0 * P, dvar_, (size_t)mc * P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      GPK_CHECK_HIP(h, hipMemcpyAsync(dvar + m0 * P * D, ddv, (size_t)mc * P * D * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    return GPK_OK;
  });
}

extern "C" int gpk_sparse_predict_grad(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var, double* dmean,
                                       double* dvar, int var_includes_noise) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, "sparse_predict_grad: no finalised sparse model (call gpk_sparse_finalize first)");
  return sparse_predict_grad(h, s, Xq, M, mean, var, dmean, dvar, var_includes_noise);
}

// The sparse mean is the mean of an exact model over (Z, alpha_u): its Hessian is gpk_predict_mean_hess on the inducing inputs.
static int sparse_predict_hess(gpk_handle h, gpk_sparse* s, const double* Xq, int64_t M, double* mean, double* dmean, double* hess) {
  GPK_REQUIRE(h, hess != nullptr, "sparse_predict_hess: hess is null");
  GPK_REQUIRE(h, Xq && mean && dmean && M >= 1, "sparse_predict_hess: null pointer or empty batch");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = s->D, P = s->P;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "sparse_predict_hess", "Xq"));
  const int64_t m = s->m;
  SparseServe sv;
  sv.fill(1, &s, 0);
  if (sv.small(h, M)) return gpk_serve_hess(h, sv.models(), true, Xq, M, mean, dmean, hess);
  // the query panels of sparse_predict_grad for the fused mean and its Jacobian (their bits); inside a panel the Hessians in
  // blocks of at most 64 MiB
  const int64_t panel = gpk_panel_rows(6ull << 30, (size_t)3 * s->mp * sizeof(double), M);
  int64_t hrows = gpk_panel_rows(64ull << 20, (size_t)P * D * D * sizeof(double), M);
  if (hrows > panel) hrows = panel;
  const size_t nq = (size_t)panel * D, nm = (size_t)panel * P, nj = nm * D, nh = (size_t)hrows * P * D * D;
  GPK_TRY(s->q.reserve(h, (nq + nm + nj + nh) * sizeof(double)));
  double *dq = s->q, *dmn = dq + nq, *ddm = dmn + nm, *dhs = ddm + nj;
  return gpk_query_panels(h, Xq, M, D * sizeof(double), panel, dq, [&](int64_t m0, int64_t mc) -> int {
    GPK_TRY(gpk_predict_mean(h, GPK_F64, s->Z, s->alpha, m, D, P, s->ls, s->sf2, s->y_mean, s->y_std, dq, mc, dmn));
    GPK_TRY(gpk_predict_mean_grad(h, s->Z, s->alpha, m, D, P, s->ls, s->sf2, s->y_std, dq, mc, ddm));
    GPK_CHECK_HIP(h, hipMemcpyAsync(mean + m0 * P, dmn, (size_t)mc * P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPK_CHECK_HIP(h, hipMemcpyAsync(dmean + m0 * P * D, ddm, (size_t)mc * P * D * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    for (int64_t r0 = 0; r0 < mc; r0 += hrows) {      // (the stream orders the blocks' launches and downloads on dhs)
      const int64_t rc = mc - r0 < hrows ? mc - r0 : hrows;
      GPK_TRY(gpk_predict_mean_hess(h, s->Z, s->alpha, m, D, P, s->ls, s->sf2, s->y_std, dq + r0 * D, rc, dhs));
      GPK_CHECK_HIP(h, hipMemcpyAsync(hess + (m0 + r0) * P * D * D, dhs, (size_t)rc * P * D * D * sizeof(double), hipMemcpyDeviceToHost,
                                      h->stream));
    }
    return GPK_OK;
  });
}

extern "C" int gpk_sparse_predict_hess(gpk_handle h, const double* Xq, int64_t M, double* mean, double* dmean, double* hess) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, "sparse_predict_hess: no finalised sparse model (call gpk_sparse_finalize first)");
  return sparse_predict_hess(h, s, Xq, M, mean, dmean, hess);
}

static int sparse_predict_cov(gpk_handle h, gpk_sparse* s, const double* Xq, int64_t M, double* mean, double* cov) {
  GPK_REQUIRE(h, Xq && mean && cov && M >= 1 && M <= 16384, "sparse_predict_cov: null pointer or M outside [1, 16384]");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = s->D, P = s->P;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "sparse_predict_cov", "Xq"));
  const int64_t m = s->m, mp = s->mp;
  std::vector<double> sig((size_t)M * M);
  SparseServe sv;
  sv.fill(1, &s, 1);
  if (sv.small(h, M)) {      // two launches
    GPK_TRY(gpk_serve_cov(h, sv.models(), true, Xq, M, mean, sig.data()));
  } else {
    // one panel: K* (training-major), the stacked panel [V0; V1] = [Wuu K*; WSigma K*] by two tile GEMMs (the inverse factors'
    // zero triangles skipped), its copy [V0; -V1], and ONE symmetric product of depth 2 mp whose epilogue forms
    // K(Xq, Xq) + noise I - (V0^T V0 - V1^T V1) and stores every tile and its transpose
    const int64_t Mp = gpk_padded(M);
    const size_t nq = (size_t)M * D, nm = (size_t)M * P, nv = (size_t)mp * Mp;
    GPK_TRY(s->q.reserve(h, (nq + nm) * sizeof(double)));
    GPK_TRY(s->work.reserve(h, (5 * nv + (size_t)Mp * Mp) * sizeof(double)));
    double *dq = s->q, *dmn = dq + nq;
    double *Kt = (double*)s->work.p, *VA = Kt + nv, *VB = VA + 2 * nv, *dcov = VB + 2 * nv;
    GPK_TRY(gpk_query_panels(h, Xq, M, D * sizeof(double), M, dq, [&](int64_t, int64_t) -> int {
      GPK_TRY(gpk_predict_mean(h, GPK_F64, s->Z, s->alpha, m, D, P, s->ls, s->sf2, s->y_mean, s->y_std, dq, M, dmn));
      GPK_CHECK_HIP(h, hipMemcpyAsync(mean, dmn, nm * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      GPK_TRY(gpk_cross_gram_t(h, GPK_F64, s->Z, m, dq, M, D, s->ls, s->sf2, Kt, Mp));
      for (int f = 0; f < 2; ++f) {
        GemmArgs g = gemm_args(f ? s->WS.p : s->Wuu.p, mp, 0, Kt, Mp, 1, VA + (size_t)f * nv, Mp, (int)mp, (int)Mp, (int)mp, 1.0, 0.0);
        g.ke0 = GPK_TILE;
        g.ke_row = GPK_TILE;
        g.k_super = 1;            // the inverse factors are zero right of the diagonal for GPK_ZERO_BAND_TILES - 1 tiles (gpk_trtri)
        g.heavy_first = 1;
        GPK_TRY(gpk_gemm(h, GPK_F64, g));
      }
      const long long tot = 2 * (long long)nv;
      hipLaunchKernelGGL(sparse_stack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, (const double*)VA,
                         (long long)mp, (long long)Mp, VB);
      GPK_LAUNCH_CHECK(h);
      GPK_TRY(gpk_cov_from_v(h, VA, VB, 2 * mp, dq, M, D, s->ls, s->sf2, s->noise, dcov, Mp));
      GPK_CHECK_HIP(h, hipMemcpy2DAsync(sig.data(), (size_t)M * sizeof(double), dcov, (size_t)Mp * sizeof(double),
                                        (size_t)M * sizeof(double), (size_t)M, hipMemcpyDeviceToHost, h->stream));
      return GPK_OK;
    }));
  }
  sv.scale_cov(sig.data(), M, cov);
  return GPK_OK;
}

extern "C" int gpk_sparse_predict_cov(gpk_handle h, const double* Xq, int64_t M, double* mean, double* cov) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, "sparse_predict_cov: no finalised sparse model (call gpk_sparse_finalize first)");
  return sparse_predict_cov(h, s, Xq, M, mean, cov);
}

// ---- the per-axis batch: B single-output sparse models on one query batch ---------------------------------------------------
namespace {

// The models of a batch entry: B (checked by the caller) finalised single-output sparse models of equal m and D on h's device.
int sparse_batch_models(gpk_handle h, const std::string& name, int B, const gpk_handle* models, gpk_sparse** list) {
  for (int b = 0; b < B; ++b) {
    GPK_REQUIRE(h, models[b], name + ": null handle in the list of models");
    gpk_sparse* s = list[b] = models[b]->sparse;
    GPK_REQUIRE(h, s && s->finalized, name + ": a model is not a finalised sparse model (call gpk_sparse_finalize first)");
    GPK_REQUIRE(h, models[b]->device == h->device, name + ": every model must live on the serving handle's device");
    GPK_REQUIRE(h, s->P == 1, name + ": every model must have one output");
    GPK_REQUIRE(h, b == 0 || (s->m == list[0]->m && s->D == list[0]->D), name + ": the models must agree in m and D");
  }
  return GPK_OK;
}

// The checks the three batch entries share, then the models taken apart.
int sparse_batch(gpk_handle h, const char* who, int B, const gpk_handle* models, const double* Xq, int64_t M, int64_t max_M,
                 int var_includes_noise, SparseServe& sb) {
  const std::string name(who);
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, name + ": 1..8 models");
  GPK_REQUIRE(h, models && Xq && M >= 1, name + ": null pointer or empty batch");
  GPK_REQUIRE(h, max_M <= 0 || M <= max_M, name + ": M outside [1, 16384]");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  gpk_sparse* list[GPK_SMALL_MAX_MODELS];
  GPK_TRY(sparse_batch_models(h, name, B, models, list));
  GPK_TRY(gpk_require_finite(h, Xq, M * list[0]->D, who, "Xq"));
  sb.fill(B, list, var_includes_noise);
  return GPK_OK;
}

}  // namespace

extern "C" int gpk_sparse_predict_multi(gpk_handle h, int B, const gpk_handle* models, const double* Xq, int64_t M, double* mean,
                                        double* var, int var_includes_noise) {
  if (!h) return GPK_BAD_ARG;
  SparseServe sb;
  GPK_TRY(sparse_batch(h, "sparse_predict_multi", B, models, Xq, M, 0, var_includes_noise, sb));
  GPK_REQUIRE(h, mean, "sparse_predict_multi: null pointer");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)B * M;
  std::vector<double> mn(n), vr(var ? n : 0);
  if (sb.small(h, M)) {
    GPK_TRY(gpk_serve_predict(h, sb.models(), true, Xq, M, mn.data(), var ? vr.data() : nullptr));
  } else {      // model by model through the panels of the single entry
    for (int b = 0; b < B; ++b)
      GPK_TRY(sparse_predict(h, sb.s[b], Xq, M, mn.data() + (size_t)b * M, var ? vr.data() + (size_t)b * M : nullptr, var_includes_noise));
  }
  gpk_interleave(mn.data(), B, M, 1, mean);
  if (var) gpk_interleave(vr.data(), B, M, 1, var);
  return GPK_OK;
}

extern "C" int gpk_sparse_predict_multi_grad(gpk_handle h, int B, const gpk_handle* models, const double* Xq, int64_t M, double* mean,
                                             double* var, double* dmean, double* dvar, int var_includes_noise) {
  if (!h) return GPK_BAD_ARG;
  SparseServe sb;
  GPK_TRY(sparse_batch(h, "sparse_predict_multi_grad", B, models, Xq, M, 0, var_includes_noise, sb));
  GPK_REQUIRE(h, mean && dmean, "sparse_predict_multi_grad: null pointer");
  GPK_REQUIRE(h, (var == nullptr) == (dvar == nullptr), "sparse_predict_multi_grad: var and dvar come together (both or neither)");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = sb.D;
  const size_t n = (size_t)B * M, nd = n * D;
  std::vector<double> mn(n), dm(nd), vr(var ? n : 0), dv(var ? nd : 0);
  if (sb.small(h, M)) {
    GPK_TRY(gpk_serve_grad(h, sb.models(), true, Xq, M, mn.data(), var ? vr.data() : nullptr, dm.data(), var ? dv.data() : nullptr));
    if (var) sb.scale_dvar(dv.data(), M, dv.data());
  } else {
    for (int b = 0; b < B; ++b)
      GPK_TRY(sparse_predict_grad(h, sb.s[b], Xq, M, mn.data() + (size_t)b * M, var ? vr.data() + (size_t)b * M : nullptr,
                                  dm.data() + (size_t)b * M * D, var ? dv.data() + (size_t)b * M * D : nullptr, var_includes_noise));
  }
  gpk_interleave(mn.data(), B, M, 1, mean);
  gpk_interleave(dm.data(), B, M, D, dmean);
  if (var) {
    gpk_interleave(vr.data(), B, M, 1, var);
    gpk_interleave(dv.data(), B, M, D, dvar);
  }
  return GPK_OK;
}

extern "C" int gpk_sparse_predict_multi_hess(gpk_handle h, int B, const gpk_handle* models, const double* Xq, int64_t M, double* mean,
                                             double* dmean, double* hess) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, hess != nullptr, "sparse_predict_multi_hess: hess is null");
  SparseServe sb;
  GPK_TRY(sparse_batch(h, "sparse_predict_multi_hess", B, models, Xq, M, 0, 0, sb));
  GPK_REQUIRE(h, mean && dmean, "sparse_predict_multi_hess: null pointer");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = sb.D;
  const size_t n = (size_t)B * M, nd = n * D, nh = nd * D;
  std::vector<double> mn(n), dm(nd), hs(nh);
  if (sb.small(h, M)) {      // every model's own inducing inputs: the model is a grid dimension of the first launch
    GPK_TRY(gpk_serve_hess(h, sb.models(), true, Xq, M, mn.data(), dm.data(), hs.data()));
  } else {
    for (int b = 0; b < B; ++b)
      GPK_TRY(sparse_predict_hess(h, sb.s[b], Xq, M, mn.data() + (size_t)b * M, dm.data() + (size_t)b * M * D,
                                  hs.data() + (size_t)b * M * D * D));
  }
  gpk_interleave(mn.data(), B, M, 1, mean);
  gpk_interleave(dm.data(), B, M, D, dmean);
  gpk_interleave(hs.data(), B, M, D * D, hess);
  return GPK_OK;
}

extern "C" int gpk_sparse_predict_multi_cov(gpk_handle h, int B, const gpk_handle* models, const double* Xq, int64_t M, double* mean,
                                            double* cov) {
  if (!h) return GPK_BAD_ARG;
  SparseServe sb;
  GPK_TRY(sparse_batch(h, "sparse_predict_multi_cov", B, models, Xq, M, 16384, 1, sb));
  GPK_REQUIRE(h, mean && cov, "sparse_predict_multi_cov: null pointer");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)B * M, nc = (size_t)M * M;
  std::vector<double> mn(n);
  if (sb.small(h, M)) {
    GPK_TRY(gpk_serve_cov(h, sb.models(), true, Xq, M, mn.data(), cov));
    sb.scale_cov(cov, M, cov);
  } else {
    for (int b = 0; b < B; ++b) GPK_TRY(sparse_predict_cov(h, sb.s[b], Xq, M, mn.data() + (size_t)b * M, cov + (size_t)b * nc));
  }
  gpk_interleave(mn.data(), B, M, 1, mean);
  return GPK_OK;
}

// ---- horizon propagation (K11) on the sparse posteriors: the chain of gpk_propagate.hip on the two-factor description ----------
// The stage's variance comes out of the two-factor launch final - times y_std^2, the noise level inside kss - in the layout of
// its var_out (M x P for one model, B x M for a batch): the advance launch takes it as it is (ystd2 = 1, add_noise = 0).
static int sparse_propagate_any(gpk_handle h, const std::string& who, int var_includes_noise, const Horizon& z) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, who + "no finalised sparse model (call gpk_sparse_finalize first)");
  GPK_REQUIRE(h, h->small_path, who + "the small-batch path is switched off (option small_path)");
  const int D = s->D, P = s->P;
  GPK_REQUIRE(h, P >= 1 && P <= GPK_PROP_MAX_NX && P <= D, who + "the state dimension P must be in [1, 16] and must not exceed D");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  SparseServe sv;
  sv.fill(1, &s, var_includes_noise);
  PropK k{};
  k.nx = P; k.D = D; k.NO = P;
  k.so = 1; k.sm = P; k.vo = 1; k.vm = P;
  for (int d = 0; d < 16; ++d) { k.in_shift[d] = 0.0; k.in_scale[d] = 1.0; k.model_of[d] = d < P ? d : -1; k.ystd2[d] = 1.0; }
  return gpk_propagate_run(h, who, sv.models(), k, z);
}

extern "C" int gpk_sparse_propagate(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U, int u_rows,
                                    const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H, double* traj,
                                    double* Sigma, double* mean, double* var, double* jac) {
  return sparse_propagate_any(h, "sparse_propagate: ", var_includes_noise,
                              Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac});
}

// ... at second order (order = 2): the mean's model is (Z, alpha_u), as in gpk_sparse_predict_hess; corr (H, R, P), may be null
extern "C" int gpk_sparse_propagate2(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U, int u_rows,
                                     const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H, double* traj,
                                     double* Sigma, double* mean, double* var, double* jac, int order, double* corr) {
  return sparse_propagate_any(h, "sparse_propagate2: ", var_includes_noise,
                              Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, order, corr});
}

// What the batch entries are called with past the handle and before the horizon.
struct SparseBatchArgs {
  int B;
  const gpk_handle* models;
  int var_includes_noise, nx;
  const int* coord;
  const double *in_shift, *in_scale, *out_shift, *out_scale;
};

static int sparse_propagate_multi_any(gpk_handle h, const char* entry, const SparseBatchArgs& a, const Horizon& z) {
  if (!h) return GPK_BAD_ARG;
  const std::string who(std::string(entry) + ": ");
  const int B = a.B, nx = a.nx;
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, who + "1..8 models");
  GPK_REQUIRE(h, a.models && a.coord, who + "null pointer");
  GPK_REQUIRE(h, h->batch == 1, who + "not available in batched mode");
  GPK_REQUIRE(h, h->small_path, who + "the small-batch path is switched off (option small_path)");
  GPK_REQUIRE(h, (a.in_shift == nullptr) == (a.in_scale == nullptr), who + "in_shift and in_scale go together");
  GPK_REQUIRE(h, (a.out_shift == nullptr) == (a.out_scale == nullptr), who + "out_shift and out_scale go together");
  gpk_sparse* list[GPK_SMALL_MAX_MODELS];
  GPK_TRY(sparse_batch_models(h, entry, B, a.models, list));
  const int D = list[0]->D;
  GPK_REQUIRE(h, D >= 1 && D <= GPK_PROP_MAX_D && nx >= B && nx <= D, who + "the state dimension nx must be in [B, D], D <= 16");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  SparseServe sb;
  sb.fill(B, list, a.var_includes_noise);
  PropK k{};
  k.nx = nx; k.D = D; k.NO = B;
  k.so = z.R; k.sm = 1; k.vo = z.R; k.vm = 1;
  for (int d = 0; d < 16; ++d) { k.in_shift[d] = 0.0; k.in_scale[d] = 1.0; k.model_of[d] = -1; k.ystd2[d] = 1.0; }
  for (int b = 0; b < B; ++b) {
    GPK_REQUIRE(h, a.coord[b] >= 0 && a.coord[b] < nx, who + "coord must be in [0, nx)");
    GPK_REQUIRE(h, k.model_of[a.coord[b]] < 0, who + "coord must be distinct");
    k.model_of[a.coord[b]] = b;
  }
  if (a.in_shift) {
    GPK_REQUIRE(h, gpk_finite(a.in_shift, D) && gpk_finite(a.in_scale, D), who + "the input scaler must not contain NaN or infinity");
    for (int d = 0; d < D; ++d) {
      GPK_REQUIRE(h, a.in_scale[d] != 0.0, who + "in_scale must be non-zero");
      k.in_shift[d] = a.in_shift[d];
      k.in_scale[d] = a.in_scale[d];
    }
    k.scaled = 1;
  }
  // the affine map behind every model's output, folded into the normalisation the kernels apply (as BatchedARDGP.propagate
  // folds it on the host): out_shift + out_scale (y_mean + y_std s)
  if (a.out_shift) {
    GPK_REQUIRE(h, gpk_finite(a.out_shift, B) && gpk_finite(a.out_scale, B), who + "the output scaler must not contain NaN or infinity");
    for (int b = 0; b < B; ++b) {
      sb.y_mean[b] = a.out_shift[b] + a.out_scale[b] * sb.y_mean[b];
      sb.y_std[b] = a.out_scale[b] * sb.y_std[b];
    }
  }
  return gpk_propagate_run(h, who, sb.models(), k, z);
}

extern "C" int gpk_sparse_propagate_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                          const int* coord, const double* in_shift, const double* in_scale, const double* out_shift,
                                          const double* out_scale, const double* x0, int x0_rows, const double* U, int u_rows,
                                          const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H,
                                          double* traj, double* Sigma, double* mean, double* var, double* jac) {
  return sparse_propagate_multi_any(h, "sparse_propagate_multi",
                                    {B, models, var_includes_noise, nx, coord, in_shift, in_scale, out_shift, out_scale},
                                    Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac});
}

// ... at second order: the output scaler folded into y_std scales c as it scales the mean; corr (H, R, B), may be null
extern "C" int gpk_sparse_propagate2_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                           const int* coord, const double* in_shift, const double* in_scale, const double* out_shift,
                                           const double* out_scale, const double* x0, int x0_rows, const double* U, int u_rows,
                                           const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H,
                                           double* traj, double* Sigma, double* mean, double* var, double* jac, int order,
                                           double* corr) {
  return sparse_propagate_multi_any(h, "sparse_propagate2_multi",
                                    {B, models, var_includes_noise, nx, coord, in_shift, in_scale, out_shift, out_scale},
                                    Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, order, corr});
}

// ... with the gradient of a horizon cost (order 1; gpk_propagate.hip: the adjoint chain): the Hessian-vector launch runs on the
// mean's model (Z, alpha_u), the variance gradient is the two-factor launch's
extern "C" int gpk_sparse_propagate_grad(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U,
                                         int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H,
                                         double* traj, double* Sigma, double* mean, double* var, double* jac, const double* gx,
                                         const double* gS, double* dU, double* dx0, double* dSigma0) {
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  return sparse_propagate_any(h, "sparse_propagate_grad: ", var_includes_noise,
                              Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, 1, nullptr, &g});
}

extern "C" int gpk_sparse_propagate_grad_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                               const int* coord, const double* in_shift, const double* in_scale,
                                               const double* out_shift, const double* out_scale, const double* x0, int x0_rows,
                                               const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                               const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                               double* jac, const double* gx, const double* gS, double* dU, double* dx0,
                                               double* dSigma0) {
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  return sparse_propagate_multi_any(h, "sparse_propagate_grad_multi",
                                    {B, models, var_includes_noise, nx, coord, in_shift, in_scale, out_shift, out_scale},
                                    Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, 1, nullptr, &g});
}

// ---- exact moment matching (K11) on the sparse posteriors: the engine of gpk_moments.hip on (Z, alpha_u, Q) --------------------
// The sparse posterior is the exact model's form over the m inducing inputs: mean weights alpha_u, and in the variance
//   Q = Wuu^T Wuu - WSigma^T WSigma  ( = (Kuu + jitter_uu I)^-1 - Sigma~ )
// where K^-1 stands, so E[v_b] = kss_b - sum_ij Q_ij L^bb_ij and every other closed form is unchanged.
namespace {

// Q (i, j) -= T (i, j) over the lower triangle j <= i < mp.  grid (ceil(mp / 256), mp), 256 threads.
__global__ __launch_bounds__(256) void sparse_q_sub_kernel(double* __restrict__ Q, const double* __restrict__ T, long long mp) {
  const long long i = blockIdx.y, j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < mp && j <= i) Q[i * mp + j] -= T[i * mp + j];
}

// Q of the assembled model s, formed on first use: two gpk_wtw products (the lower tiles, ld = mp) and the subtraction, on h's
// stream, which is drained - the next call may come through another serving handle.  Rows and columns >= m hold I - I = 0 and
// are masked by the pair kernel anyway.
int sparse_moment_matrix(gpk_handle h, gpk_sparse* s) {
  if (s->q_ready) return GPK_OK;
  const int64_t mp = s->mp;
  const size_t mm = (size_t)mp * mp;
  if (!s->Qm) GPK_TRY(s->Qm.alloc(h, mm));
  gpk_dev<double> T;
  GPK_TRY(T.alloc(h, mm));
  GPK_TRY(gpk_wtw(h, s->Wuu, mp, mp, s->Qm, mp));
  GPK_TRY(gpk_wtw(h, s->WS, mp, mp, T, mp));
  hipLaunchKernelGGL(sparse_q_sub_kernel, dim3((unsigned)((mp + 255) / 256), (unsigned)mp), dim3(256), 0, h->stream, s->Qm.p,
                     (const double*)T.p, (long long)mp);
  GPK_LAUNCH_CHECK(h);
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));      // (T leaves scope)
  s->q_ready = true;
  return GPK_OK;
}

// What the four entries share: the handle rules of the sparse propagate siblings, then the models taken apart as the engine's
// description (sm.m, which points into sm) - kss = sf2 (+ the noise level), floor 0 and no separate noise term, as the exact
// Python callers pass them; the output scaler folded into y_mean / y_std.  models null: the object of h itself, P outputs.
// check(D): the entry's own refusals - the engine's, made here as well so that a refused call does not even form Q.
struct SparseMoments {
  SparseServe sv;
  const double* Qp[GPK_SMALL_MAX_MODELS];
  HostModels m;
};

template <class Check>
int sparse_moments_models(gpk_handle h, const std::string& who, int B, const gpk_handle* models, int var_includes_noise, int nx,
                          const int* coord, const double* in_shift, const double* in_scale, const double* out_shift,
                          const double* out_scale, bool chain, Check check, SparseMoments& sm) {
  GPK_REQUIRE(h, h->batch == 1, who + "not available in batched mode");
  GPK_REQUIRE(h, h->small_path, who + "the small-batch path is switched off (option small_path)");
  gpk_sparse* list[GPK_SMALL_MAX_MODELS];
  if (models) {
    GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, who + "1..8 models");
    GPK_REQUIRE(h, (in_shift == nullptr) == (in_scale == nullptr), who + "in_shift and in_scale go together");
    GPK_REQUIRE(h, (out_shift == nullptr) == (out_scale == nullptr), who + "out_shift and out_scale go together");
    GPK_TRY(sparse_batch_models(h, who.substr(0, who.size() - 2), B, models, list));
  } else {
    list[0] = h->sparse;
    GPK_REQUIRE(h, list[0] && list[0]->finalized, who + "no finalised sparse model (call gpk_sparse_finalize first)");
  }
  const int D = list[0]->D, NO = B * list[0]->P;
  GPK_REQUIRE(h, D >= 1 && D <= GPK_PROP_MAX_D && nx >= 1 && nx <= GPK_PROP_MAX_NX && nx <= D, who + "needs 1 <= nx <= D <= 16");
  GPK_REQUIRE(h, !chain || nx >= NO, who + "the state dimension nx must not be below the number of outputs");
  GPK_REQUIRE(h, list[0]->mp <= GPK_SMALL_MAX_NP, who + "needs m <= 16384");
  if (chain && coord) {
    bool seen[GPK_PROP_MAX_NX] = {false};
    for (int b = 0; b < B; ++b) {
      GPK_REQUIRE(h, coord[b] >= 0 && coord[b] < nx, who + "coord must be in [0, nx)");
      GPK_REQUIRE(h, !seen[coord[b]], who + "coord must be distinct");
      seen[coord[b]] = true;
    }
  }
  if (in_shift) {
    GPK_REQUIRE(h, gpk_finite(in_shift, D) && gpk_finite(in_scale, D), who + "the input scaler must not contain NaN or infinity");
    for (int d = 0; d < D; ++d) GPK_REQUIRE(h, in_scale[d] != 0.0, who + "in_scale must be non-zero");
  }
  if (out_shift)
    GPK_REQUIRE(h, gpk_finite(out_shift, B) && gpk_finite(out_scale, B), who + "the output scaler must not contain NaN or infinity");
  GPK_TRY(check(D));
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  sm.sv.fill(B, list, var_includes_noise);
  for (int b = 0; b < B; ++b) {
    GPK_TRY(sparse_moment_matrix(h, list[b]));
    sm.Qp[b] = list[b]->Qm;
    if (out_shift) {
      sm.sv.y_mean[b] = out_shift[b] + out_scale[b] * sm.sv.y_mean[b];
      sm.sv.y_std[b] = out_scale[b] * sm.sv.y_std[b];
    }
  }
  const SparseServe& sv = sm.sv;
  sm.m = HostModels{B, sv.P, sv.Z, sv.alpha, sv.m, D, sv.ls, sv.sf2, sv.y_mean, sv.y_std, sm.Qp, sv.mp, sv.mp, sv.kss, 0.0, 0, nullptr,
                    nx, coord, in_shift, in_scale};
  return GPK_OK;
}

// the query entries' own refusals (those of gpk_mm_query, made before Q is formed)
int sparse_moments_query_check(gpk_handle h, const std::string& who, int D, int nx, const double* Xq, const double* Sq, int M,
                               const double* mean, const double* cov, const double* xcov) {
  GPK_REQUIRE(h, M >= 1 && M <= GPK_SMALL_MAX_M, who + "M must be in [1, 32]");
  GPK_REQUIRE(h, Xq && mean && cov && xcov, who + "null pointer");
  GPK_REQUIRE(h, gpk_finite(Xq, (size_t)M * D), who + "the queries must not contain NaN or infinity");
  GPK_REQUIRE(h, !Sq || gpk_finite(Sq, (size_t)M * nx * nx), who + "the covariances must not contain NaN or infinity");
  return GPK_OK;
}

}  // namespace

extern "C" int gpk_sparse_moments(gpk_handle h, int var_includes_noise, int nx, const double* Xq, const double* Sq, int M,
                                  double* mean, double* cov, double* xcov) {
  if (!h) return GPK_BAD_ARG;
  const std::string who("sparse_moments: ");
  SparseMoments sm;
  GPK_TRY(sparse_moments_models(h, who, 1, nullptr, var_includes_noise, nx, nullptr, nullptr, nullptr, nullptr, nullptr, false,
                                [&](int D) { return sparse_moments_query_check(h, who, D, nx, Xq, Sq, M, mean, cov, xcov); }, sm));
  return gpk_mm_query(h, who, sm.m, Xq, Sq, M, mean, cov, xcov);
}

extern "C" int gpk_sparse_moments_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                        const double* in_shift, const double* in_scale, const double* out_shift,
                                        const double* out_scale, const double* Xq, const double* Sq, int M, double* mean,
                                        double* cov, double* xcov) {
  if (!h) return GPK_BAD_ARG;
  const std::string who("sparse_moments_multi: ");
  GPK_REQUIRE(h, models, who + "null pointer");
  SparseMoments sm;
  GPK_TRY(sparse_moments_models(h, who, B, models, var_includes_noise, nx, nullptr, in_shift, in_scale, out_shift, out_scale, false,
                                [&](int D) { return sparse_moments_query_check(h, who, D, nx, Xq, Sq, M, mean, cov, xcov); }, sm));
  return gpk_mm_query(h, who, sm.m, Xq, Sq, M, mean, cov, xcov);
}

extern "C" int gpk_sparse_propagate_mm(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U,
                                       int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H,
                                       double* traj, double* Sigma, double* mean, double* cov, double* xcov) {
  if (!h) return GPK_BAD_ARG;
  const std::string who("sparse_propagate_mm: ");
  Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean};
  z.cov = cov; z.xcov = xcov;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, who + "no finalised sparse model (call gpk_sparse_finalize first)");
  const int P = s->P;
  GPK_REQUIRE(h, P >= 1 && P <= GPK_PROP_MAX_NX && P <= s->D, who + "the state dimension P must be in [1, 16] and must not exceed D");
  SparseMoments sm;
  GPK_TRY(sparse_moments_models(h, who, 1, nullptr, var_includes_noise, P, nullptr, nullptr, nullptr, nullptr, nullptr, true,
                                [&](int D) { return gpk_horizon_check(h, who, P, D, z); }, sm));
  return gpk_mm_chain(h, who, sm.m, z);
}

extern "C" int gpk_sparse_propagate_mm_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                             const int* coord, const double* in_shift, const double* in_scale,
                                             const double* out_shift, const double* out_scale, const double* x0, int x0_rows,
                                             const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                             const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* cov,
                                             double* xcov) {
  if (!h) return GPK_BAD_ARG;
  const std::string who("sparse_propagate_mm_multi: ");
  GPK_REQUIRE(h, models && coord, who + "null pointer");
  Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean};
  z.cov = cov; z.xcov = xcov;
  SparseMoments sm;
  GPK_TRY(sparse_moments_models(h, who, B, models, var_includes_noise, nx, coord, in_shift, in_scale, out_shift, out_scale, true,
                                [&](int D) { return gpk_horizon_check(h, who, nx, D, z); }, sm));
  return gpk_mm_chain(h, who, sm.m, z);
}

// ---- ... with the adjoint of the moments: gpk_mm_query_vjp / gpk_mm_chain_grad on the same (Z, alpha_u, Q).  The engine's own
// refusals of the seeds and results are made here as well, ahead of Q; the chains ask for the tape (gpk_moments.hip).
namespace {

int sparse_moments_vjp_check(gpk_handle h, const std::string& who, int D, int NO, int nx, const double* Xq, const double* Sq, int M,
                             const double* mean, const double* cov, const double* xcov, const double* gmean, const double* gcov,
                             const double* gxcov, const double* dXq, const double* dSq) {
  GPK_TRY(sparse_moments_query_check(h, who, D, nx, Xq, Sq, M, mean, cov, xcov));
  GPK_REQUIRE(h, dXq && dSq, who + "null result dXq or dSq");
  const size_t n_om = (size_t)M * NO;
  GPK_REQUIRE(h, (!gmean || gpk_finite(gmean, n_om)) && (!gcov || gpk_finite(gcov, n_om * NO)) && (!gxcov || gpk_finite(gxcov, n_om * D)),
              who + "the seeds gmean, gcov and gxcov must not contain NaN or infinity");
  return GPK_OK;
}

int sparse_moments_grad_check(gpk_handle h, const std::string& who, int nx, int D, const Horizon& z) {
  GPK_TRY(gpk_horizon_check(h, who, nx, D, z));
  const HorizonGrad& g = *z.grad;
  GPK_REQUIRE(h, g.gx && g.dx0, who + "null seed gx or null result dx0");
  GPK_REQUIRE(h, D == nx || g.dU, who + "null result dU");
  GPK_REQUIRE(h, gpk_finite(g.gx, (size_t)(z.H + 1) * z.R * nx) && (!g.gS || gpk_finite(g.gS, (size_t)(z.H + 1) * z.R * nx * nx)),
              who + "the seeds gx and gS must not contain NaN or infinity");
  return GPK_OK;
}

}  // namespace

extern "C" int gpk_sparse_moments_vjp(gpk_handle h, int var_includes_noise, int nx, const double* Xq, const double* Sq, int M,
                                      double* mean, double* cov, double* xcov, const double* gmean, const double* gcov,
                                      const double* gxcov, double* dXq, double* dSq) {
  if (!h) return GPK_BAD_ARG;
  const std::string who("sparse_moments_vjp: ");
  SparseMoments sm;
  GPK_TRY(sparse_moments_models(h, who, 1, nullptr, var_includes_noise, nx, nullptr, nullptr, nullptr, nullptr, nullptr, false,
                                [&](int D) {
                                  return sparse_moments_vjp_check(h, who, D, h->sparse->P, nx, Xq, Sq, M, mean, cov, xcov, gmean, gcov,
                                                                  gxcov, dXq, dSq);
                                }, sm));
  return gpk_mm_query_vjp(h, who, sm.m, Xq, Sq, M, mean, cov, xcov, gmean, gcov, gxcov, dXq, dSq);
}

extern "C" int gpk_sparse_moments_vjp_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                            const double* in_shift, const double* in_scale, const double* out_shift,
                                            const double* out_scale, const double* Xq, const double* Sq, int M, double* mean,
                                            double* cov, double* xcov, const double* gmean, const double* gcov, const double* gxcov,
                                            double* dXq, double* dSq) {
  if (!h) return GPK_BAD_ARG;
  const std::string who("sparse_moments_vjp_multi: ");
  GPK_REQUIRE(h, models, who + "null pointer");
  SparseMoments sm;
  GPK_TRY(sparse_moments_models(h, who, B, models, var_includes_noise, nx, nullptr, in_shift, in_scale, out_shift, out_scale, false,
                                [&](int D) {
                                  return sparse_moments_vjp_check(h, who, D, B, nx, Xq, Sq, M, mean, cov, xcov, gmean, gcov, gxcov,
                                                                  dXq, dSq);
                                }, sm));
  return gpk_mm_query_vjp(h, who, sm.m, Xq, Sq, M, mean, cov, xcov, gmean, gcov, gxcov, dXq, dSq);
}

extern "C" int gpk_sparse_propagate_mm_grad(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U,
                                            int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q, int R,
                                            int H, double* traj, double* Sigma, double* mean, double* cov, double* xcov,
                                            const double* gx, const double* gS, double* dU, double* dx0, double* dSigma0) {
  if (!h) return GPK_BAD_ARG;
  const std::string who("sparse_propagate_mm_grad: ");
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean};
  z.cov = cov; z.xcov = xcov; z.grad = &g;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, who + "no finalised sparse model (call gpk_sparse_finalize first)");
  const int P = s->P;
  GPK_REQUIRE(h, P >= 1 && P <= GPK_PROP_MAX_NX && P <= s->D, who + "the state dimension P must be in [1, 16] and must not exceed D");
  SparseMoments sm;
  GPK_TRY(sparse_moments_models(h, who, 1, nullptr, var_includes_noise, P, nullptr, nullptr, nullptr, nullptr, nullptr, true,
                                [&](int D) { return sparse_moments_grad_check(h, who, P, D, z); }, sm));
  return gpk_mm_chain_grad(h, who, sm.m, z, true);
}

extern "C" int gpk_sparse_propagate_mm_grad_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                                  const int* coord, const double* in_shift, const double* in_scale,
                                                  const double* out_shift, const double* out_scale, const double* x0, int x0_rows,
                                                  const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                                  const double* Q, int R, int H, double* traj, double* Sigma, double* mean,
                                                  double* cov, double* xcov, const double* gx, const double* gS, double* dU,
                                                  double* dx0, double* dSigma0) {
  if (!h) return GPK_BAD_ARG;
  const std::string who("sparse_propagate_mm_grad_multi: ");
  GPK_REQUIRE(h, models && coord, who + "null pointer");
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean};
  z.cov = cov; z.xcov = xcov; z.grad = &g;
  SparseMoments sm;
  GPK_TRY(sparse_moments_models(h, who, B, models, var_includes_noise, nx, coord, in_shift, in_scale, out_shift, out_scale, true,
                                [&](int D) { return sparse_moments_grad_check(h, who, nx, D, z); }, sm));
  return gpk_mm_chain_grad(h, who, sm.m, z, true);
}

extern "C" int gpk_sparse_export(gpk_handle h, int64_t* m, int* D, int* P, int* n_ls, double* Z, double* G, double* g, double* yy,
                                 int64_t* n_rows, double* ls, double* hyper, double* y_mean, double* y_std) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s, "sparse_export: no sparse model");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  if (m) *m = s->m;
  if (D) *D = s->D;
  if (P) *P = s->P;
  if (n_ls) *n_ls = s->n_ls;
  if (n_rows) *n_rows = s->n_rows;
  if (ls) for (int d = 0; d < s->n_ls; ++d) ls[d] = s->ls_in[d];
  if (hyper) { hyper[0] = s->sf2; hyper[1] = s->noise; hyper[2] = s->jitter; hyper[3] = s->jitter_uu; }
  for (int p = 0; p < s->P; ++p) {
    if (y_mean) y_mean[p] = s->y_mean[p];
    if (y_std) y_std[p] = s->y_std[p];
  }
  const size_t pitch = (size_t)s->nt * sizeof(double), mrow = (size_t)s->m * sizeof(double);
  if (Z) GPK_CHECK_HIP(h, hipMemcpyAsync(Z, s->Z, (size_t)s->m * s->D * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (G) GPK_CHECK_HIP(h, hipMemcpy2DAsync(G, mrow, s->S, pitch, mrow, (size_t)s->m, hipMemcpyDeviceToHost, h->stream));
  std::vector<double> gt, yt;
  if (g) {      // rows mp .. mp + P - 1 of S hold g^T
    gt.resize((size_t)s->P * s->m);
    GPK_CHECK_HIP(h, hipMemcpy2DAsync(gt.data(), mrow, s->S + (size_t)s->mp * s->nt, pitch, mrow, (size_t)s->P,
                                      hipMemcpyDeviceToHost, h->stream));
  }
  if (yy) {
    yt.resize((size_t)s->P);
    GPK_CHECK_HIP(h, hipMemcpy2DAsync(yt.data(), sizeof(double), s->S + (size_t)s->mp * s->nt + s->mp, pitch + sizeof(double),
                                      sizeof(double), (size_t)s->P, hipMemcpyDeviceToHost, h->stream));
  }
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  if (g)
    for (int64_t j = 0; j < s->m; ++j)
      for (int p = 0; p < s->P; ++p) g[j * s->P + p] = gt[(size_t)p * s->m + j];
  if (yy) for (int p = 0; p < s->P; ++p) yy[p] = yt[(size_t)p];
  return GPK_OK;
}

extern "C" int gpk_sparse_import(gpk_handle h, const double* Z, int64_t m, int D, int P, const double* ls, int n_ls, double sf2,
                                 double noise, double jitter, double jitter_uu, const double* y_mean, const double* y_std,
                                 const double* G, const double* g, const double* yy, int64_t n_rows) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, G && g && yy && n_rows >= 0, "sparse_import: null pointer or negative row count");
  if (m >= 1 && m <= SP_MAX_M && P >= 1 && P <= GPK_MAX_P) {
    GPK_TRY(gpk_require_finite(h, G, m * m, "sparse_import", "G"));
    GPK_TRY(gpk_require_finite(h, g, m * P, "sparse_import", "g"));
    GPK_TRY(gpk_require_finite(h, yy, P, "sparse_import", "yy"));
  }
  gpk_sparse* s = nullptr;
  GPK_TRY(sparse_new(h, Z, m, D, P, ls, n_ls, sf2, noise, jitter, jitter_uu, y_mean, y_std, &s));
  // S (zeroed by sparse_new): G, then g as the targets' rows and columns, yy on their diagonal (the cross moments of
  // different outputs are not part of the model: they stay zero)
  const size_t pitch = (size_t)s->nt * sizeof(double), mrow = (size_t)m * sizeof(double);
  std::vector<double> gt((size_t)P * m);
  for (int64_t j = 0; j < m; ++j)
    for (int p = 0; p < P; ++p) gt[(size_t)p * m + j] = g[j * P + p];
  GPK_CHECK_HIP(h, hipMemcpy2DAsync(s->S, pitch, G, mrow, mrow, (size_t)m, hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemcpy2DAsync(s->S + (size_t)s->mp * s->nt, pitch, gt.data(), mrow, mrow, (size_t)P, hipMemcpyHostToDevice,
                                    h->stream));
  GPK_CHECK_HIP(h, hipMemcpy2DAsync(s->S + s->mp, pitch, g, (size_t)P * sizeof(double), (size_t)P * sizeof(double), (size_t)m,
                                    hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemcpy2DAsync(s->S + (size_t)s->mp * s->nt + s->mp, pitch + sizeof(double), yy, sizeof(double),
                                    sizeof(double), (size_t)P, hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  s->n_rows = n_rows;
  return GPK_OK;
}

// The path set of the assembled model (K10, the sparse models): the model taken apart for gpk_paths_prepare_two (gpk_paths.hip).
extern "C" int gpk_sparse_paths_prepare(gpk_handle h, const double* Omega, const double* phase, int64_t F, const double* W_rand,
                                        const double* Xi, int S, double* Coef, int64_t ldc, double* Zdst) {
  if (!h) return GPK_BAD_ARG;
  gpk_sparse* s = h->sparse;
  GPK_REQUIRE(h, s && s->finalized, "sparse_paths_prepare: no finalised sparse model (call gpk_sparse_finalize first)");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  return gpk_paths_prepare_two(h, s->Z, s->m, s->D, s->P, s->sf2, s->Wuu, s->WS, s->mp, s->alpha, Omega, phase, F, W_rand, Xi, S,
                               Coef, ldc, Zdst);
}
