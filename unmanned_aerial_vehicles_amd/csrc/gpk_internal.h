// Internal declarations shared by the libgpk translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gpk.h"

struct gpk_model;    // the composite calls' model (gpk_model.hip)
struct gpk_bmodel;   // B single-output models on shared inputs (gpk_fit_batched, gpk_bmodel.hip)
struct gpk_sparse;   // the sparse inducing-point model (gpk_sparse_begin, gpk_sparse.hip)

struct gpk_context {
  int device = 0;
  gpk_model* model = nullptr;        // owned: gpk_fit / gpk_import create it, gpk_destroy / gpk_model_release free it
  gpk_bmodel* bmodel = nullptr;      // owned: gpk_fit_batched creates it, gpk_destroy / gpk_model_release free it
  gpk_sparse* sparse = nullptr;      // owned: gpk_sparse_begin / gpk_sparse_import create it, gpk_destroy / gpk_model_release free it
  hipStream_t stream = nullptr;      // stream kernels are launched on
  hipStream_t own_stream = nullptr;  // created by gpk_create
  bool user_stream = false;
  std::string err;
  // growable device scratch owned by the handle (small / medium temporaries)
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  int* d_info = nullptr;        // device int for potrf pivot failures
  double* h_small = nullptr;    // 4 KiB of pinned, device-mapped host memory: the reductions' results (LML terms, gradient sums, status words)
  double* d_small = nullptr;    // ... its device address: the kernels write there, the host reads h_small after the synchronisation - no copy command
  unsigned* d_count = nullptr;  // 2 x 8 zero-initialised ticket counters (last-workgroup reductions, gpk_small.hip)
  unsigned* d_cov_count = nullptr;   // zero-initialised ticket counters of the small covariance reduction (allocated on first use)
  // staging of the one-call serving entries (gpk_serve.hip): device block [Xq | work] and pinned, mapped host block [Xq | outputs]
  void* serve_dev = nullptr;
  size_t serve_dev_bytes = 0;
  void* serve_host = nullptr;
  size_t serve_host_bytes = 0;
  int gemm_small_tiles = 1024;   // launches with fewer 128 x 128 tiles than this run on 64 x 64 tiles
  int gemm_tiny_tiles = 320;     // fp64 launches with fewer 128 x 128 tiles than this run on 32 x 32 tiles (option gemm_tiny_tiles; 0: never);
                                 // measured (profiles/r05_gemm_tiny_ab.log): W^T W at N = 1024 59 -> 33 us, 2048 108 -> 84 us, trtri 1024 117 -> 74 us;
                                 // with 1024 the products of N >= 4096 lose
  int gemm_balanced = 1;         // launches whose tiles differ in k-range: balanced persistent tile schedule
  long long gemm_balanced_max_tiles = 32768;   // ... up to this many tiles per launch (all problems of a batch)
  int cus = 0;                   // compute units of the device (read once: gpk_cus)
  int moments_query_groups = 0;  // moment matching's pair launch: groups of queries as a grid dimension (0: as many as bring the launch to
                                 // two workgroups per CU, gpk_moments.hip; n >= 1: at most n, so 1 is the launch without the split)
  int moments_tape_mb = 1024;    // the moment chain's gradient, where the caller asks for the tape (the sparse entries): the stages' work
                                 // blocks are kept, 5 H + 4 H launches, while H blocks fit this many MiB (0: never; a memory cap)
  int trtri_levels = 1;      // gpk_trtri: one batched launch per level for power-of-two tile counts
  int trsm256 = 1;           // potrf: fused 256-wide base of the triangular solve
  int small_path = 1;        // gpk_predict_host: two-launch small-batch kernels (option small_path = 0 disables)
  int k3_stream_min_np = 512;    // gpk_potrs_inv: streaming matrix-vector passes from this padded size up (P <= 6); measured faster than the two
                                 // 128-column tile GEMMs from there on (N = 4096: 0.11 against 0.35 ms, profiles/r04_k3_ab.log)
  int k5_split2_tile = 0;    // fp16 x 2 variance launch: 0 = the tallest tile (512 / 256 / 128 x 128) that still comes in >= 512
                             // tiles; 1 = always 128 x 128; 2 = 512 x 128 whenever Np % 512 == 0; 3 = 256 x 128 whenever Np % 256 == 0
  int k5_mfma_shape = 0;     // ... its MFMA shape: 0 = the default (gpk_k5split.hip), 1 = 32x32x16, 2 = 16x16x32
  int ptile = 1;             // gpk_potrf: one persistent launch (gpk_ptile.hip) for 512 <= Np <= ptile_max_np
  int ptile_max_np = 24576;  // (above, the recursion: halves that are one launch each + GEMMs.  One launch against that at 20 480 rows 46.7 / 48.6 ms,
                             // 24 576 78.6 / 79.2, 32 768 179.4 / 172.5, 40 960 347.4 / 340.6: profiles/r05_ptile_large.log; 16 384 until round 5)
  int ptile_prog_max_nt = 128;  // ... up to this many tile columns the two tiles under a diagonal tile follow that tile's factorisation 16
                             // columns at a time instead of waiting for the whole inverse (0: never)
  int ptile_inv_max_np = 4608;  // gpk_lml_eval: up to this padded size the inverse factor's tiles are tasks of the same launch (0: never)
  int ptile_prog_rows = 8;   // ... how many tiles under the diagonal one do so (1 .. 8).  Measured (profiles/r05_ptile_followers_ab.log): N = 4096
                             // 1.69 ms with none, 1.37 with one, 1.22 with two, 1.18 with four, 1.15 with eight, the same with twelve / sixteen
  int* d_ptile = nullptr;    // its ticket counter, abort word and per-tile-row progress counters
  int ptile_slots = 512;     // workgroups that fit the device at two per CU
  int ptile_sr = 1, ptile_sr_max_nt = 36;   // ... and up to this many tile columns the 256-register build (two k-tiles in flight in the off-diagonal
                             // k-loops: gpk_ptile.hip, SR); ptile_sr = 0: the 128-register build for everything
  int ptile_single_max_nt = 96;   // ... up to this many tile columns the launch keeps ONE workgroup per CU
  int ptile_launches = 0;    // one-launch factorisations issued by the current gpk_potrf (their abort words are checked at its end)
  std::string ptile_trace_request;   // option "ptile_trace_path" (debugging aid): the NEXT one-launch factorisation writes its per-task time stamps there
  std::string ptile_trace_path;   // ... while that launch is in flight
  long long ptile_trace_n = 0;
  int sparse_panel = 0;      // gpk_sparse_update / gpk_sparse_accumulate: rows per panel (0: F = [Kfu | Yn] within 128 MiB, 1024 .. 16384 rows)
  int sparse_slabs = 0;      // ... k-slabs of a panel's product F^T F (0: a function of (mp, panel rows), gpk_sparse.hip; 1 .. 64)
  int fitc_fused = 1;        // the weighted (FITC) pass: q_i from ONE tile GEMM on the panel F (0: gpk_predict_var_inv on the panel's rows, the check)
  int debug_fill = 0;        // option debug_fill: the handle's scratch is overwritten with 0xFF bytes (NaN) at every request
  int gemm_log = 0;          // option gemm_log = 1: log every tile-GEMM launch to stderr (profiling aid)
  int gram_log = 0;          // option gram_log = 1: log the form of every gpk_gram / gpk_predict_mean[_multi] / gpk_predict_mean_mfma launch and of every small-batch serving call to stderr
  int k5_log = 0;            // option k5_log = 1: log the form of every 16-bit variance launch (gpk_k5split.hip) to stderr
  // gpk_timing: HIP-event brackets around the dominant launches (K5 variance GEMM, K1 Gram kernel), a ring of pairs
  struct TimedLaunch { hipEvent_t e0 = nullptr, e1 = nullptr; int tag = 0; };
  int timing = 0;
  std::vector<TimedLaunch> timed;   // GPK_TIMING_RING entries once enabled
  long long timed_count = 0;        // launches bracketed so far (ring position = count % size)
  // batched mode (gpk_batch_begin .. gpk_batch_end): `batch` same-shaped problems per call.  Pointers passed
  // to the entry points address problem 0; a pointer that falls inside a registered buffer advances by that
  // buffer's stride per problem, any other pointer is shared by all problems.
  struct BatchBuf { const char* base; long long stride; };
  int batch = 1;
  std::vector<BatchBuf> bbufs;
};

#define GPK_CHECK_HIP(h, call)                                                          \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
      return GPK_HIP_ERROR;                                                             \
    }                                                                                   \
  } while (0)

#define GPK_REQUIRE(h, cond, msg)                                                       \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      (h)->err = std::string("bad argument: ") + (msg);                                 \
      return GPK_BAD_ARG;                                                               \
    }                                                                                   \
  } while (0)

#define GPK_LAUNCH_CHECK(h)                                                             \
  do {                                                                                  \
    hipError_t e_ = hipGetLastError();                                                  \
    if (e_ != hipSuccess) {                                                             \
      (h)->err = std::string("kernel launch: ") + hipGetErrorString(e_);                \
      return GPK_HIP_ERROR;                                                             \
    }                                                                                   \
  } while (0)

#define GPK_TRY(expr)                                                                   \
  do {                                                                                  \
    int rc_ = (expr);                                                                   \
    if (rc_ != GPK_OK) return rc_;                                                      \
  } while (0)

int gpk_scratch(gpk_handle h, size_t bytes, void** out);
// compute units of the handle's device, read once (256 where the runtime does not say)
inline int gpk_cus(gpk_handle h) {
  if (h->cus <= 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus <= 0) cus = 256;
    h->cus = cus;
  }
  return h->cus;
}

// ---- one-launch tile Cholesky (gpk_ptile.hip) -----------------------------------------
constexpr size_t GPK_PTILE_CTRL_INTS = 16 + 8 * 512 + 1024 + 10 * 8 * 512;   // ticket, abort, padding; GPK_MAX_BATCH x (Np / 128 <= 512) row
                                                        // counters; one pause word per CU; per tile row: 16-column steps of the diagonal
                                                        // tile / of the tile left of it / of the tile left of that one published so far
// *used = 1: the launch was issued (the caller synchronises, reads info and calls gpk_potrf_ptile_check); 0: not served
// wband / ldw (optional): the band of zeros right of the diagonal tiles of this matrix is written by the launch's own preparation
// (gpk_trtri's zero_band_kernel, for the caller that goes on to the inverse factor); zero_info: so are the pivot words
int gpk_potrf_ptile(gpk_handle h, double* A, int64_t Np, int64_t lda, double* winv, int row0, int* used, double* wt = nullptr,
                    double* wband = nullptr, int64_t ldw = 0, int zero_info = 0);
int gpk_potrf_ptile_check(gpk_handle h, int gave_up = -1);
void gpk_model_free(gpk_handle h);   // gpk_model.hip: all three models of the handle
void gpk_bmodel_free(gpk_handle h);  // gpk_bmodel.hip
void gpk_sparse_free(gpk_handle h);  // gpk_sparse.hip
// the body of gpk_sparse_paths_prepare (gpk_paths.hip): a path set from the sparse model's Z, two inverse factors and alpha_u
int gpk_paths_prepare_two(gpk_handle h, const double* Z, int64_t m, int D, int P, double sf2, const double* Wuu, const double* WS,
                          int64_t mp, const double* alpha, const double* Omega, const double* phase, int64_t F,
                          const double* W_rand, const double* Xi, int S, double* Coef, int64_t ldc, double* Zdst);
// the launches of gpk_potrf / gpk_lml_terms / gpk_lml_grad without their synchronisations (gpk_lml_eval)
int gpk_potrf_enqueue(gpk_handle h, double* A, int64_t Np, int64_t lda, double* winv);
int gpk_potrf_finish(gpk_handle h, const int* hinfo_all, int* info, int gave_up = -1);
// status words of an evaluation chain: ints [0, 8] of h->d_small + GPK_STATUS_OFF receive the pivot failures (h->batch ints) and the
// one-launch factorisation's "gave up" flag (written by the terms launch: gpk_lml_terms_enqueue(..., with_status = 1))
constexpr int GPK_STATUS_OFF = 480;
// max |(float)W_ij| over the lower triangle per 128-row block, as float bits (first pass of gpk_split2_rows_f64)
int gpk_tril_block_absmax_f64_enqueue(gpk_handle h, const double* W, int64_t n, int64_t ld, unsigned* out);
int gpk_potrf_trtri_enqueue(gpk_handle h, double* A, int64_t Np, int64_t lda, double* winv, double* W, int64_t ldw, double* wt,
                            int* used);   // factor + inverse factor as one persistent launch (small matrices), or *used = 0
int gpk_lml_terms_enqueue(gpk_handle h, const double* L, int64_t N, int64_t ldl, const double* Y, const double* alpha, int P,
                          double* dout, int with_status = 0);   // with_status: + the chain's status words, in the same launch
int gpk_lml_grad_enqueue(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2, const double* alpha,
                         int P, const double* Kinv, int64_t ldk, double* dout);
// B single-output evaluations on shared X as ONE chain with ONE synchronisation (gpk_lml_batched): the buffers hold the B
// problems one behind the other (K, W, Kinv: Np * Np doubles apart; winv: Np * 128; T: tsz; Yn, alpha: Ne).  K holds the
// Gram matrices on entry.  terms[2 b .. 2 b + 1], grads[b * (D + 2) ..] (gpk_lml_grad's order), info[b] (pivot failures).
int gpk_lml_chain_batched(gpk_handle h, int B, const double* X, int64_t N, int D, const double* ls /* B x D */, const double* sf2,
                          const double* noise, const double* Yn, int64_t Ne, double* K, int64_t Np, double* winv, double* W,
                          double* T, size_t tsz, double* alpha, double* Kinv, double* terms, double* grads, int* info);

// Event brackets of gpk_timing (no-ops unless enabled): record the first event, launch, record the second.
constexpr int GPK_TIMING_RING = 64;
inline void gpk_time_begin(gpk_handle h, int tag) {
  if (!h->timing) return;
  auto& t = h->timed[(size_t)(h->timed_count % GPK_TIMING_RING)];
  t.tag = tag;
  (void)hipEventRecord(t.e0, h->stream);
}
inline void gpk_time_end(gpk_handle h) {
  if (!h->timing) return;
  auto& t = h->timed[(size_t)(h->timed_count % GPK_TIMING_RING)];
  (void)hipEventRecord(t.e1, h->stream);
  ++h->timed_count;
}

// byte stride between consecutive problems of a batch for the buffer `p` points into (0: shared / not batched)
inline long long gpk_bstride(gpk_handle h, const void* p) {
  if (h->batch <= 1) return 0;
  const char* c = (const char*)p;
  for (const auto& b : h->bbufs)
    if (c >= b.base && c < b.base + b.stride) return b.stride;
  return 0;
}

// ---- dense GEMM on MFMA (gpk_gemm.hip) ---------------------------------------------
// C[m x n] = alpha * opA(A) * opB(B)^T + beta * C on whole 128x128 tiles.
//   ta == 0: A stored (m x k), k contiguous;  ta == 1: A stored (k x m), m contiguous.
//   tb == 0: B stored (n x k), k contiguous;  tb == 1: B stored (k x n), n contiguous.
// m, n multiples of 128; k multiple of 16.  lower_only skips tiles strictly above the
// diagonal.  Per-tile k range: [kb0 + kb_row * tile_row + kb_col * tile_col,
// ke0 + ke_row * tile_row + ke_col * tile_col) clipped to [0, k) (ke0 < 0 means "k").
// tiles from the diagonal tile rightwards that gpk_trtri / gpk_tril_to_f32 zero; a k_super launch may read that far
// beyond a row's own k-range (a super-tile spans at most two bands of 8 tile rows)
constexpr int GPK_ZERO_BAND_TILES = 16;

constexpr int GPK_GRAD_W = 17;   // doubles per tile written by epilogue 4, and per COLUMN of a tile by epilogue 5

struct GemmArgs {
  const void* A;
  const void* B;
  void* C;
  int64_t lda, ldb, ldc;
  int m, n, k;
  int ta, tb;
  double alpha, beta;
  int lower_only;
  int kb0, kb_row, kb_col, ke0, ke_row, ke_col;
  int heavy_first;  // process tile rows in reverse order (use when the k-range grows with the tile row)
  int k_super;      // every row of an 8-row super-tile takes the k-range of its longest row (the operand must be
                    // zero beyond each row's own range): the 64 workgroups of a super-tile then run in lockstep
  int epilogue;   // 0: store C;  1: C (fp64, ld = ldc) [tile_row][col] = sum over the tile's rows of (alpha*acc)^2
                  // 2: store C (beta = 0) and atomicMax |(float)C_ij| into amax[128-row block of the matrix at amax_base, ld = ldc]
                  // 3: fp64, ta = tb = 1, lower_only, m == n: C_ij = C_ji = cov_sf2 exp(-|u_i - u_j|^2 / 2) + cov_noise [i == j] - acc_ij
                  //    with u = cov_q (cov_m x cov_d, the queries divided by the length-scales); i or j >= cov_m: -acc_ij
                  // 4: fp64, ta = 0, tb = 1, every tile: nothing of the product Q = A B is stored; C (fp64) [tile_row * (n / tile) + tile_col][17]
                  //    = sum over the tile of Q_ni A_ni ((x_nd - z_id) / ls_d)^2 for d < grad_d (entries [0, 16)) and of Q_ni A_ni ([16]),
                  //    x = grad_x (grad_n x grad_d, rows of A), z = grad_z (grad_m x grad_d, columns of C); A's first n columns are read back
                  // 5: the operands of 4; C (fp64) [tile_row * (n / tile) + tile_col][column of the tile][17] = sum over the tile's ROWS of
                  //    Q_ni A_ni (x_nd / ls_d - z_id / ls_d) for d < grad_d (entries [0, 16)) and of Q_ni A_ni ([16])
  unsigned* amax;
  const void* amax_base;
  const double* cov_q;
  double cov_sf2, cov_noise;
  int cov_d, cov_m;
  const double* grad_x;
  const double* grad_z;
  int grad_n, grad_m, grad_d;
  double grad_ls[16];
  // nbatch > 0: that many independent products in one launch (second grid dimension), operand i at base + i * stride
  // (bytes); in the handle's batched mode every problem of the batch runs all of them.
  int nbatch;
  long long sA, sB, sC;
};
inline GemmArgs gemm_args(const void* A, int64_t lda, int ta, const void* B, int64_t ldb, int tb,
                          void* C, int64_t ldc, int m, int n, int k, double alpha, double beta) {
  GemmArgs g{};
  g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.m = m; g.n = n; g.k = k; g.ta = ta; g.tb = tb; g.alpha = alpha; g.beta = beta;
  g.lower_only = 0; g.kb0 = 0; g.kb_row = 0; g.kb_col = 0; g.ke0 = -1; g.ke_row = 0; g.ke_col = 0; g.epilogue = 0; g.heavy_first = 0; g.k_super = 0;
  g.nbatch = 0; g.sA = 0; g.sB = 0; g.sC = 0; g.amax = nullptr; g.amax_base = nullptr;
  g.cov_q = nullptr; g.cov_sf2 = 0.0; g.cov_noise = 0.0; g.cov_d = 0; g.cov_m = 0;
  return g;
}
int gpk_gemm(gpk_handle h, int dtype, const GemmArgs& g);
int gpk_gemm_tile(gpk_handle h, const GemmArgs& g);   // 128 or 64: the tile edge gpk_gemm will pick

// ---- small-batch serving kernels (gpk_small.hip) -------------------------------------
// M <= 32 fp64 queries against B models x P outputs each (B > 1: P == 1, the per-axis batch), all models on one query batch.
constexpr int GPK_SMALL_MAX_M = 32;          // queries per call
constexpr int64_t GPK_SMALL_MAX_NP = 16384;  // padded training rows
constexpr int GPK_SMALL_MAX_MODELS = 8;      // single-output models served by one call
constexpr int GPK_SMALL_COV_COUNTERS = GPK_SMALL_MAX_MODELS * 129 + GPK_SMALL_MAX_MODELS;
                                             // h->d_cov_count: ticket counters of the covariance's two-level reduction, per model
                                             // 1 + GPK_SMALL_MAX_NP / 16 / 16 = 65, in the two-factor form 1 + 2 * 64 = 129 (one
                                             // top-level count and the groups of both factors); the last GPK_SMALL_MAX_MODELS are
                                             // small_wtv_grad_kernel's, one per model
// What a serving call runs on: B <= GPK_SMALL_MAX_MODELS models x P outputs each (B > 1: P == 1) of equal N and D, each with its
// own inputs, alpha, kernel and normalisation, and F inverse factors per model.  F = 1: the exact GP and the per-axis batch,
// variance terms kss - |W[0] k*|^2.  F = 2: the sparse model on its inducing inputs (gpk_sparse.hip), kss - |W[0] k*|^2 +
// |W[1] k*|^2 with W[0] = Wuu, W[1] = WSigma.  A member that the call at hand does not read may be null.
struct ServeModels {
  int B, P, F;
  const double* const* X;         // B device pointers (N x D)
  const double* const* alpha;     // B device pointers (N x P)
  int64_t N;
  int D;
  const double* ls;               // B x D
  const double* sf2;              // B
  const double *y_mean, *y_std;   // B * P
  const double* const* W[2];      // per factor B device pointers (Np x ldw, 16-byte aligned): variance, gradient, covariance
  int64_t Np, ldw;                // Np = gpk_padded(N), even ldw >= Np (read with W)
  const double* kss;              // B: the prior variance the variance starts from
  double floor_;                  // ... and the level it is clipped at
  const double* noise;            // B: the level on the covariance's diagonal
};
// The results of a call; null: not requested.  mean (B, M, P) and dmean (B, M, P, D) un-normalised.  var: F = 1 (B, M) in
// normalised-target units, F = 2 (B, M, P) already multiplied by y_std^2.  dvar (B, M, D) and cov (B, M, M): normalised-target
// units in both forms.  var and dvar come together in a gradient call.
struct ServeOut {
  double *mean, *var, *dmean, *dvar, *cov;
  double* hess;      // (B, M, P, D, D) un-normalised, every D x D block symmetric bit for bit (GPK_SMALL_HESS)
};
bool gpk_small_ok(int64_t Np, int D, int P, int64_t M);
// doubles of device work area (`work`) that a call of the given kind needs: per model K* (32 x Np) + the workgroups' shares
// (F inverse factors per model: K*, the mean and the Jacobian shares stay one set per model)
enum { GPK_SMALL_PREDICT, GPK_SMALL_COV, GPK_SMALL_GRAD, GPK_SMALL_JACVAR, GPK_SMALL_HESS };
size_t gpk_small_work_doubles(int call, int64_t Np, int B, int64_t M, int D, int P, int F);
// The launches of one call on M <= GPK_SMALL_MAX_M queries, no synchronisation; Xq and the outputs may be pinned, mapped host
// memory.  The launch counts are those of one model with one output for every B, P and F:
//   GPK_SMALL_PREDICT  mean: 1 launch; with out.var 2
//   GPK_SMALL_GRAD     mean + dmean: 1 launch; with out.var and out.dvar 3
//   GPK_SMALL_COV      mean + cov (m.noise on the diagonal, not clipped): 2 launches
//   GPK_SMALL_JACVAR   mean + dmean + var (a stage of the propagation chains, gpk_propagate_run): 2 launches, the bits of GPK_SMALL_GRAD's
//   GPK_SMALL_HESS     mean + dmean + hess (no inverse factor is read; out.var / out.dvar null): GPK_SMALL_GRAD's one launch, untouched
//                      (its bits), then small_hess_kernel: 2 launches
// Block b of every output has the bits of model b served alone.
int gpk_small_launch(gpk_handle h, int call, const ServeModels& m, const double* Xq, int64_t M, double* work, const ServeOut& out);
// The trace launch of a second-order propagation stage (small_hess_trace_kernel): the workgroups' shares of tr(H_o Sg_m) for the
// M device query rows Xq, each with its own nx x nx covariance Sg[m] (device, raw units; in_scale: D host values, the queries'
// scaler).  groups = gpk_small_trace_groups(Np) workgroups per model write shares[(g * E + e) * 2 + {0, 1}], E = B M P and
// e = (b * M + m) * P + p, and trs[b * M + m]; tr(H Sg) = y_std (sum_g shares[..0] - trs * sum_g shares[..1]).  No inverse
// factor is read (F = 1 or 2), nothing is synchronised, and no other launch's results are read.
unsigned gpk_small_trace_groups(int64_t Np);
int gpk_small_trace_launch(gpk_handle h, const ServeModels& m, const double* Xq, int64_t M, const double* Sg, int nx,
                           const double* in_scale, double* shares, double* trs);
// The Hessian-vector launch of a backward propagation stage (small_hvp_kernel): the workgroups' shares of H_o w_o for the M
// device query rows Xq, H_o the mean's input Hessian of output o per unit of the RAW query, never formed.  w_o = [G[coord of o,
// :nx], 0] with G = Lam A Sg per query row, A = I + lin[:, :nx] + the stage's Jacobian rows: the workgroups form their own rows
// of G from what the chain keeps on the device.  groups = gpk_small_trace_groups(Np) workgroups per model write
// shares[(g * E + e) * D + d], E = B M P, e = (b * M + m) * P + p; H_o w_o = sum_g shares.  No ticket, no atomics, no inverse
// factor (F = 1 or 2), nothing is synchronised.
struct SmallHvp {
  const double *Lam, *Sg;            // device, M x nx x nx each: the adjoint of the next stage's covariance, this stage's covariance
  const double *sjac, *lin;          // device: the stage's Jacobians (output o, row m at [(o * so + m * sm) * D + d]), lin (nx x D)
  int nx, so, sm, scaled;
  int model_of[16];                  // state coordinate -> output, or -1
  int coord_of[16];                  // output -> state coordinate
  double in_scale[16];               // the queries' scaler (ones without)
};
int gpk_small_hvp_launch(gpk_handle h, const ServeModels& m, const double* Xq, int64_t M, const SmallHvp& c, double* shares);
// ---- horizon propagation (gpk_propagate.hip): what the entries of the exact models and of the sparse models (gpk_sparse.hip) share
constexpr int GPK_PROP_MAX_R = GPK_SMALL_MAX_M, GPK_PROP_MAX_H = 256, GPK_PROP_MAX_NX = 16, GPK_PROP_MAX_D = 16;
// The composition's parameters.  Output o of the stage (a single model's output p, or model b of a batch) sits at
// smean[o * so + m * sm], svar[o * vo + m * vm] and sjac[(o * so + m * sm) * D + d] for query row m.  One-factor models: svar in
// normalised-target units (ystd2, noise, add_noise apply); two-factor models: svar is final (ystd2 = 1, add_noise = 0).
struct PropK {
  int nx, D, NO;                     // state width, query width, outputs of a stage
  int so, sm, vo, vm;
  int model_of[GPK_PROP_MAX_NX];     // state coordinate -> the output that drives it, or -1 (lin alone, no variance)
  int scaled;                        // the queries go through (q - in_shift) / in_scale, the Jacobians through 1 / in_scale
  double in_shift[GPK_PROP_MAX_D], in_scale[GPK_PROP_MAX_D];
  double ystd2[16];                  // y_std[o]^2: the variance in target units is svar * ystd2, as the Python layer forms it
  double noise[16];                  // added to svar (normalised units) when the variance is to include the noise level
  int add_noise;
};
// The seeds and results of the adjoint chain: gx (H + 1, R, nx) = dl/dx_h, gS (H + 1, R, nx, nx) = dl/dSigma_h (null: zero; the
// chain uses (gS + gS^T) / 2); dU (R, H, nu) (null when nu = 0), dx0 (R, nx), dSigma0 (R, nx, nx) (may be null).
struct HorizonGrad {
  const double *gx, *gS;
  double *dU, *dx0, *dSigma0;
};
// What the entries share past their model arguments.
struct Horizon {
  const double *x0, *U, *lin, *Sigma0, *Q;
  int x0_rows, u_rows, s_rows, R, H;
  double *traj, *Sigma, *mean, *var, *jac;
  int order = 1;                     // 2: the mean takes c_o = tr(H_o Sigma_h) / 2 per stage, added last (see gpk_propagate.hip)
  double* corr = nullptr;            // (H, R, NO): c of every stage, zeros at order 1; may be null
  const HorizonGrad* grad = nullptr;   // the gradient of a horizon cost (order 1 only): the backward sweep follows the chain
  double *cov = nullptr, *xcov = nullptr;   // the moment chain's stage outputs (H, R, NO, NO) and (H, R, NO, D); null elsewhere
};
// What the host entries of the exact models are called with past the handle and before the horizon (the single-model entries: B = 1
// and pointers to their scalars).  W, ldw: the inverse factors; in the moment entries (gpk_moments.hip) K^-1 and its leading dimension.
struct HostModels {
  int B, P;
  const double* const* X;
  const double* const* alpha;
  int64_t N;
  int D;
  const double *ls, *sf2, *y_mean, *y_std;
  const double* const* W;
  int64_t Np, ldw;
  const double* kss;
  double floor_;
  int var_includes_noise;
  const double* noise;
  int nx;
  const int* coord;                  // B state coordinates (batch) or null (single model: output p drives coordinate p)
  const double *in_shift, *in_scale;
};
inline bool gpk_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(p[i] - p[i] == 0.0)) return false;
  return true;
}
// ---- the one skeleton of every horizon chain (gpk_propagate.hip; the moment chain of gpk_moments.hip runs on it too) ----------
// What a stage's composing launch reads and writes besides the stage's own results, for the workgroup of rollout r: the stage's
// controls u + r u_row_stride and the next stage's; the state x (R x nx) and S (R x nx x nx), updated in place; qnext, the next
// stage's scaled queries (R x D), null at the last stage; the horizon's output slots of this stage; the stage's optional outputs
// out[0..2] - mean, var, jac (the moment chain: mean, cov, xcov) - null where not requested.  x null: no stage to compose.
struct StageView {
  const double *lin, *Qn, *u, *u_next;
  long long u_row_stride;
  double *x, *S, *qnext, *traj_next, *sig_next;
  double* out[3];
};
// The device block of a horizon, sized and carved by the same calls: with base null, take() only counts.  head(): the one
// upload's head [x | S | q | lin | Q | U]; outputs(): traj and Sigma from slot 1 on (slot 0 is the caller's own start) and the
// optional stage outputs, n_out[i] doubles per stage for the caller's host_out[i].  A chain's own buffers are further take()s.
struct HorizonBlock {
  int nx, D, nu, R, H;
  size_t n_x, n_s, n_q, n_lin, n_Q, n_u;
  long long u_row_stride;            // between the rollouts' control sequences; 0: one sequence serves them all
  double* base = nullptr;
  size_t at = 0;
  double *x, *S, *q, *lin, *Q, *u, *traj, *sig, *out[3];
  double* qs = nullptr;              // the scaled queries of stages 1 .. H - 1 where a chain keeps them (stage 0: q); null: q is reused
  size_t n_out[3];
  double* host_out[3];
  HorizonBlock(int nx, int D, const Horizon& z);
  double* take(size_t n) {
    double* p = base ? base + at : nullptr;
    at += n;
    return p;
  }
  void head();
  void outputs(size_t n0, double* h0, size_t n1, double* h1, size_t n2, double* h2);
  double* queries(int s) const { return s == 0 || !qs ? q : qs + (size_t)(s - 1) * n_q; }
  size_t n_head() const { return n_x + n_s + n_q + n_lin + n_Q + n_u; }
};
// lay(): every take of a chain, run twice - counting, then on the handle's scratch block of that size
template <class F>
int gpk_horizon_carve(gpk_handle h, HorizonBlock& b, F&& lay) {
  lay();
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, b.at * sizeof(double), &ws));
  b.base = (double*)ws;
  b.at = 0;
  lay();
  return GPK_OK;
}
// Every check past the model's own: R in [1, 32], H in [1, 256], row counts of 1 or R, the null pointers (U null only when nu = 0),
// NaN or infinity in x0, U, lin, Q or Sigma0.  GPK_BAD_ARG with a message, before anything is launched or written.
int gpk_horizon_check(gpk_handle h, const std::string& who, int nx, int D, const Horizon& z);
// The head of the one upload into hx (zero-initialised, n_head() doubles): the start rows (one row serves every rollout), Sigma0
// mirrored from its lower triangle, the first stage's scaled queries, lin, Q and U as they come from the host.
void gpk_horizon_pack(const HorizonBlock& b, const Horizon& z, bool scaled, const double* in_shift, const double* in_scale, double* hx);
// Slot 0 of traj and Sigma from the packed head, and the one upload (host: the head and whatever the chain packed behind it).
int gpk_horizon_upload(gpk_handle h, const HorizonBlock& b, const Horizon& z, const std::vector<double>& host);
StageView gpk_horizon_stage(const HorizonBlock& b, const Horizon& z, int s);
// The downloads of traj, Sigma and the requested stage outputs, then the chain's own, then the one synchronisation.
struct HorizonCopy {
  double* dst;
  const double* src;
  size_t n;
};
int gpk_horizon_finish(gpk_handle h, const HorizonBlock& b, const Horizon& z, std::initializer_list<HorizonCopy> more);
// The chain of one horizon on the models m (F = 1 or 2): every check of the limits (GPK_BAD_ARG before anything is launched), one
// upload, 3 H launches (order 2: 4 H, the trace launch before the advance), up to five downloads (six with corr), one
// synchronisation.  With z.grad: 6 H launches - forward the three of GPK_SMALL_GRAD and the advance, backward the
// Hessian-vector launch and propagate_adjoint_kernel - the seeds in the one upload, up to three more downloads, still one
// synchronisation; traj and Sigma keep the bits of the chain without it.
// k: nx, D, NO, the strides, model_of, the scaler, ystd2 and the noise filled in by the entry; `who` prefixes
// the messages.
int gpk_propagate_run(gpk_handle h, const std::string& who, const ServeModels& m, PropK k, const Horizon& z);
// Exact moment matching (gpk_moments.hip) on the models m - X, alpha and, as W, the matrix that stands for K^-1 in E[v] (lower
// tiles as gpk_wtw writes them, ldw its leading dimension): K^-1 of an exact model, Q = Kuu^-1 - Sigma~ of a sparse one on its
// inducing inputs (gpk_sparse.hip).  Every check of m and of the queries or the horizon (GPK_BAD_ARG before anything is launched),
// then five launches per batch of M <= 32 Gaussian queries: gpk_mm_query one upload, three downloads and one synchronisation;
// gpk_mm_chain the horizon on the skeleton above, 5 H launches and one synchronisation (z.cov, z.xcov: the stage outputs).
int gpk_mm_query(gpk_handle h, const std::string& who, const HostModels& m, const double* Xq, const double* Sq, int M, double* mean,
                 double* cov, double* xcov);
int gpk_mm_chain(gpk_handle h, const std::string& who, const HostModels& m, const Horizon& z);
// ... with the adjoint of the moments (gpk_moments.hip, "the adjoint"), on the same models - exact today, (Z, alpha_u, Q) of a sparse
// model without new kernels.  gpk_mm_query_vjp: gpk_mm_query (mean, cov, xcov keep its bits) with the seeds gmean (M x NO), gcov (M x
// NO x NO) and gxcov (M x NO x D), null: zero, and the results dXq (M x D), dSq (M x nx x nx, symmetric bit for bit); ten launches,
// one upload, one synchronisation.  gpk_mm_chain_grad: gpk_mm_chain (its bits) with z.grad - six launches per stage forward, seven
// backward, one upload, one synchronisation; with tape (the sparse entries) and H work blocks within option moments_tape_mb every
// stage keeps its block: five forward, four backward, the same bits.  A non-finite seed or a null result: GPK_BAD_ARG before anything
// is launched.
int gpk_mm_query_vjp(gpk_handle h, const std::string& who, const HostModels& m, const double* Xq, const double* Sq, int M, double* mean,
                     double* cov, double* xcov, const double* gmean, const double* gcov, const double* gxcov, double* dXq, double* dSq);
int gpk_mm_chain_grad(gpk_handle h, const std::string& who, const HostModels& m, const Horizon& z, bool tape = false);
// ... as one-call serving (gpk_serve.hip): host queries in, host results out through the pinned, mapped block, one
// synchronisation.  small: the launches above (gpk_serve_predict: 33..64 queries the same twice); otherwise, F = 1 only, the
// general chain, which also reads m.Np / m.ldw only with the inverse factor.
int gpk_serve_predict(gpk_handle h, const ServeModels& m, bool small, const double* Xq_host, int64_t M, double* mean_host,
                      double* var_host);
int gpk_serve_cov(gpk_handle h, const ServeModels& m, bool small, const double* Xq_host, int64_t M, double* mean_host,
                  double* cov_host);
int gpk_serve_grad(gpk_handle h, const ServeModels& m, bool small, const double* Xq_host, int64_t M, double* mean_host,
                   double* var_host, double* dmean_host, double* dvar_host);
// mean (B, M, P), dmean (B, M, P, D) with the bits of gpk_serve_grad's, and the mean's input Hessian (B, M, P, D, D).  small:
// GPK_SMALL_HESS, two launches for all models; otherwise one upload and the general blocks, model by model.  No inverse factor
// is read (F = 1 or 2)
int gpk_serve_hess(gpk_handle h, const ServeModels& m, bool small, const double* Xq_host, int64_t M, double* mean_host,
                   double* dmean_host, double* hess_host);
// Sigma (Mp x ldc, symmetric bit for bit) = K(Xq, Xq) + noise I - VA^T VB from two operands (rows x Mp each, ld Mp) whose
// product is symmetric (gpk_cov.hip: the covariance epilogue of the tile GEMM; VA == VB: the exact model's covariance)
int gpk_cov_from_v(gpk_handle h, const double* VA, const double* VB, int64_t rows, const double* Xq, int64_t M, int D,
                   const double* ls, double sf2, double noise, double* cov, int64_t ldc);

// K* straight into the fragment-order fp16 x 2 split layout (gpk_gram.hip); D <= 16
int gpk_cross_split2(gpk_handle h, const float* Xq, int64_t M, const float* X, int64_t N, int D, const double* ls,
                     double sf2, double scale, void* dst);
int gpk_var_finalize(gpk_handle h, const double* ss, int64_t M, double kss, double floor_, double* var);
int gpk_colsum_reduce(gpk_handle h, const double* partial, int S, int64_t Mp, double* out);
int gpk_colsum_finalize(gpk_handle h, const double* partial, int S, int64_t Mp, int64_t M, double kss, double floor_,
                        double* var);   // both of the above in one launch (entries M..Mp of var are left alone)
int gpk_colsum_finalize_packed(gpk_handle h, const double* partial, int S, int64_t Mp, int64_t M, double kss, double floor_,
                               const float* mean, int P, const double* y_std, double recheck_below, unsigned* low_count,
                               double* out);   // + [mean | var y_std^2] rows
