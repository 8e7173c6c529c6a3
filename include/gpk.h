/*
 * gpk.h — C ABI of libgpk.so: MI355X (gfx950) kernels for the Gaussian-Process
 * residual-model path of Grandediw/Unmanned_Aerial_Vehicles.
 *
 * The reference has no FFI boundary: its GP arithmetic is Python calling
 * scikit-learn / SciPy (LAPACK) on the CPU.  Each entry point below replaces one
 * of those CPU call sites (cited per function as <file>:<line> relative to the
 * reference tree; `sklearn/` = scikit-learn 1.7.2, the library the reference
 * delegates to).  The Python host side (unmanned_aerial_vehicles_amd/) binds these
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - All matrices are row-major.  "dev" pointers are device (HBM) addresses, e.g.
 *     torch.Tensor.data_ptr() on ROCm; "host" pointers are ordinary host memory.
 *   - Dense factor matrices are padded: Np = gpk_padded(N) = N rounded up to 128.
 *     The Gram kernel fills the padding with the identity, so the Cholesky factor of
 *     the padded matrix is [L 0; 0 I] and every dense kernel runs on whole tiles.
 *   - dtype: GPK_F32 or GPK_F64 selects the element type of the void* buffers.
 *   - Calls are asynchronous on the handle's stream unless stated otherwise;
 *     gpk_synchronize() waits.  Functions with a host output parameter synchronise.
 *   - Return codes: GPK_OK, GPK_NOT_PD (Cholesky pivot <= 0; 1-based row in the
 *     error string and *info), GPK_BAD_ARG, GPK_HIP_ERROR.  gpk_last_error() gives text.
 *   - No global state; one handle per GPU / host thread.  Kernels launch on, and allocations come from, the calling
 *     thread's current HIP device: gpk_set_stream (and every allocation the handle makes) selects the handle's device,
 *     so a caller that drives handles on several GPUs from one thread calls gpk_set_stream before each group of calls.
 */
#ifndef GPK_H
#define GPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpk_context* gpk_handle;

/* the exported entry points (libgpk.so is built with -fvisibility=hidden: nothing else leaves the library) */
#define GPK_API __attribute__((visibility("default")))

enum { GPK_F32 = 0, GPK_F64 = 1 };
enum { GPK_OK = 0, GPK_NOT_PD = 1, GPK_BAD_ARG = 2, GPK_HIP_ERROR = 3 };
/* GPK_MAX_D: features accepted by the Gram kernels (gpk_gram, gpk_cross_gram_t and with them gpk_predict_var*).
 * GPK_MAX_D_PREDICT: features accepted by the fused mean, the one-call serving kernels and the gradient -
 * gpk_predict_mean*, gpk_predict_host*, gpk_lml_grad - and therefore by the composite gpk_fit / gpk_predict /
 * gpk_lml and by the Python host side (the reference's largest model has 16 inputs,
 * quadrotor_gp_mpc/quadrotor_gp_mpc/gaussian_process.py:66).                                                   */
enum { GPK_TILE = 128, GPK_MAX_D = 64, GPK_MAX_D_PREDICT = 16, GPK_MAX_P = 16, GPK_MAX_BATCH = 8 };

/* ---- context ------------------------------------------------------------------ */
GPK_API int gpk_create(gpk_handle* h, int device);
GPK_API void gpk_destroy(gpk_handle h);
GPK_API const char* gpk_last_error(gpk_handle h);
/* Launch on `stream` (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream; NULL is HIP's
 * default stream).  GPK_OWN_STREAM selects the non-blocking stream created by gpk_create, which is
 * what a fresh handle uses.                                                                      */
#define GPK_OWN_STREAM ((void*)(intptr_t)-1)
GPK_API int gpk_set_stream(gpk_handle h, void* stream);
GPK_API int gpk_synchronize(gpk_handle h);
GPK_API int64_t gpk_padded(int64_t n);

/* ---- measurement aid -----------------------------------------------------------------------------------
 * gpk_timing(h, 1): from now on the handle brackets its dominant launches with HIP events recorded on the
 * handle's stream - tag GPK_TIMED_K5: the one GEMM launch of gpk_predict_var_inv / gpk_predict_var_inv_split
 * (V = W K*^T with the column-norm epilogue); tag GPK_TIMED_GRAM: the Gram kernel of gpk_gram; tag GPK_TIMED_GRAD: the
 * streaming pass of gpk_lml_grad over K^-1; tag GPK_TIMED_POTRF: the launches of one gpk_potrf; tag GPK_TIMED_COV: the
 * symmetric product (K(Xq, Xq) + noise I - V^T V) of gpk_predict_cov_inv / gpk_predict_cov; tag GPK_TIMED_JAC: the second
 * triangular product (C = W^T V) of gpk_predict_var_grad_inv; tag GPK_TIMED_PROPAGATE: the advance launch of every stage of
 * gpk_propagate_host[_multi] and gpk_sparse_propagate[_multi] - and keeps the
 * last 64 pairs.  gpk_kernel_times synchronises the stream and returns the elapsed milliseconds of the bracketed
 * launches with that tag still in the ring, oldest first (*n_out of them, at most max_n).  bench.py uses it to
 * report the dominant kernel's duration over exactly the timed steps; rocprofv3's kernel trace of the same run is
 * the cross-check.  No reference counterpart (the reference has no instrumentation on this path).        */
/* gpk_set_option: the handle's tuning knobs (the library reads NOTHING from the environment), settable on a live handle:
 * "k5_split2_tile" (gpk_predict_var_inv_split2: 0 = the tallest of the 512 / 256 / 128 x 128 tiles that still comes in at
 * least 512 tiles, 1 = always 128 x 128, 2 = 512 x 128 whenever Np % 512 == 0, 3 = 256 x 128 whenever Np % 256 == 0 and as 0
 * otherwise), "k5_mfma_shape" (the same launch: 1 = on v_mfma_f32_32x32x16_f16, 2 = on v_mfma_f32_16x16x32_f16, 0 or anything else =
 * the library's default, 16x16x32; with "k5_log" the launch names its shape on a line "GPKSHAPE ..."), "small_path", "trsm256",
 * "trtri_levels", "gemm_small_tiles" / "gemm_tiny_tiles" (launches of fewer 128 x 128 tiles than these - 1024 / 320 - run on 64 x 64 /,
 * fp64 only, 32 x 32 tiles; bit-identical results), "k3_stream_min_np", "ptile" (gpk_potrf: 1 = the one-launch tile factorisation of
 * gpk_ptile.hip for 512 <= Np <= "ptile_max_np" (24576), 0 = the recursive launch chain), "ptile_prog_max_nt" (that launch:
 * up to this many tile columns (128 = always) the tiles under a diagonal tile follow its factorisation 16 columns at a time,
 * 0 = they wait for the whole inverse tile), "ptile_prog_rows" (1 .. 8 such tiles per column; 8), "ptile_single_max_nt" (up to this many tile
 * columns (96) the launch keeps one workgroup per CU instead of two, 0 = always two), "ptile_sr" / "ptile_sr_max_nt" (1: launches of up to
 * that many tile columns (36) run the 256-register build with two k-tiles in flight; bit-identical factors), "ptile_inv_max_np" (gpk_lml_eval
 * with a gradient: up to this padded size (4608) the tiles of the inverse factor are tasks of the same launch, 0 = always the
 * level-by-level products of gpk_trtri; same values to rounding), "gemm_balanced" (tile GEMMs whose tiles differ in k-range - the
 * products with triangular operands of gpk_trtri / gpk_wtw / gpk_potrs_inv: 1 = the balanced persistent tile schedule, 0 = the
 * static tile mapping; bit-identical results), "gemm_balanced_max_tiles", "gemm_log" (1: every tile-GEMM launch to stderr),
 * "gram_log" (1: the form of every gpk_gram launch - `GPKGRAM f64|f32 N Np D strip|sym gsG ntT gridNNN` - and of every gpk_predict_mean /
 * gpk_predict_mean_multi launch - `GPKMEAN f64|f32 N M D P|B d4 p4 granG sS chunkC` - and of every gpk_predict_mean_mfma call -
 * `GPKMEANMM bf16|f32 N M D P qbQ nqbN sS chunkC`: the kernel (bf16 x 3 for D <= 14, fp32 MFMA for D = 15, 16), Q query blocks of 32
 * per wave, N workgroups of 128 Q queries, S training chunks of C points - and of every small-batch serving call (up to 32 queries) -
 * `GPKSMALL predict|cov|grad|jacvar|hess B F Np M D P gaA gbB nmbK rcR hgH slS`: models, inverse factors, A and B workgroups of the
 * first and of the factor launches, K query blocks of 16 (0: no factor launch), R row chunks of the W^T V launch, H x S workgroups x
 * slices of the Hessian launch (0: not launched) - and of every launch pair (kernel + reduction, one per query panel) of the large-batch
 * derivative entries gpk_predict_mean_grad[_multi], gpk_predict_var_grad_inv and gpk_predict_mean_hess[_multi] -
 * `GPKDERIV mean_grad|mean_grad_multi|var_grad|mean_hess|mean_hess_multi N D P|B mc d4K ps|bsG ngN nrbR nqb|ncbQ granG sS chunkC`: mc
 * queries in the panel, the D4 = K and PS | BS = G instantiation, N output or model groups x R row blocks of the Hessian's triangle
 * (the third grid dimension), Q query blocks, S training chunks of C rows, C a multiple of G (var_grad: P = 1, ps1 ng1 nrb1,
 * query blocks of 128 columns, gran 64) - and of every batch of Gaussian queries of the moment-matching entries, K11 (a query call, or
 * one stage of a chain; the backward sweep of a gradient entry writes one `adj` line per stage) -
 * `GPKMM fwd|adj B P D nx N R cusC gG uU nqQ splitS nrwW nvV pP|pcP`: R queries, C the handle's CU count, G workgroups per pair x U
 * pairs x Q groups of queries in the pair launch (S = 1: the kernel with the query dimension), W row blocks of 256, V sums per slot
 * (fwd: 1 + P (P + 1) / 2, adj: 1 + D + nx (nx + 1) / 2), the forward pair kernel's P or the adjoint's alpha-tile capacity PC -
 * to stderr, one line per launch),
 * "k5_log" (1: the form of every 16-bit variance launch - gpk_predict_var_inv_split2 / gpk_predict_mean_var_split2: `GPKK5 direct rowsR
 * ntmTA ntnB nstS padP gridG`, gpk_predict_var_inv_split: `GPKK5 split rowsR ntmTA ntnB nstS pad0 gridG`; R the tile's rows, A x B tiles,
 * S super-tiles, P tile slots per band of the walk - to stderr, one line per launch),
 * "sparse_panel" / "sparse_slabs" (the statistics pass of the sparse model, K9:
 * rows per panel and k-slabs per panel product; 0 = the built-in rule), "fitc_fused" (the weighted pass of the FITC model, K9: 1,
 * the default = the q_i from one tile GEMM on the panel, 0 = from gpk_predict_var_inv on the panel's rows, the check), "moments_query_groups" (the pair launch of the moment-matching
 * entries, K11: 0 = as many groups of queries as bring it to two workgroups per CU, n >= 1 = at most n, 1 = no split; bit-identical
 * results), "moments_tape_mb" (the gradient chains of the sparse moment entries keep every stage's work block while H blocks fit this
 * many MiB, 9 H launches instead of 13 H: default 1024, 0 = never; bit-identical results), "debug_fill" (1: the handle's scratch and serving work area are overwritten with NaN bytes at every request - the test
 * suite runs with it).  Used by the A/B timings and by the tests that pin a fast path to its plain form.
 * gpk_set_option_str: "ptile_trace_path" - the NEXT one-launch factorisation writes its per-task time stamps to that file
 * (debugging aid, tools/exp_ptile_trace.py).                                                                          */
GPK_API int gpk_set_option(gpk_handle h, const char* name, int value);
GPK_API int gpk_set_option_str(gpk_handle h, const char* name, const char* value);
enum { GPK_TIMED_K5 = 1, GPK_TIMED_GRAM = 2, GPK_TIMED_GRAD = 3, GPK_TIMED_POTRF = 4, GPK_TIMED_COV = 5, GPK_TIMED_JAC = 6,
       GPK_TIMED_SPARSE_STATS = 7, GPK_TIMED_SPARSE_PASS = 8, GPK_TIMED_PROPAGATE = 9 };
GPK_API int gpk_timing(gpk_handle h, int enable);
GPK_API int gpk_kernel_times(gpk_handle h, int tag, double* ms, int max_n, int* n_out);

/* ---- batched mode: `count` (<= 8) same-shaped problems per call --------------------------------------
 * Between gpk_batch_begin and gpk_batch_end, gpk_potrf, gpk_leaf_inverses, gpk_trtri, gpk_wtw and
 * gpk_potrs_inv work on `count` independent problems with ONE launch chain: every kernel of the chain
 * gets a batch grid dimension.  The pointer arguments address problem 0; a pointer that lies inside a
 * buffer registered with gpk_batch_buffer(base, stride_bytes) advances by that stride per problem, any
 * other pointer is shared by all problems.  gpk_potrf's `info` then receives `count` entries.
 * (BASELINE configuration 5: the per-axis ax/ay/az GPs of src/px4/gp_trainer.py:139-179 factorised
 * together.)                                                                                          */
GPK_API int gpk_batch_begin(gpk_handle h, int count);
GPK_API int gpk_batch_buffer(gpk_handle h, const void* base, int64_t stride_bytes);
GPK_API int gpk_batch_end(gpk_handle h);
GPK_API const char* gpk_version(void);

/* ---- K1: RBF Gram build ---------------------------------------------------------
 * K[i][j] = sf2 * exp(-0.5 * sum_d ((x_id - x_jd) / ls_d)^2), exact differences,
 * diagonal = sf2 + diag_add, padding rows/cols (>= N) = identity.  Symmetric tiles are
 * computed once and written to both halves.
 * Replaces: sklearn/gaussian_process/kernels.py:1553-1560 (RBF.__call__, pdist + exp +
 * squareform), :1402 (WhiteKernel diag), sklearn/gaussian_process/_gpr.py:347 (alpha
 * jitter); quadrotor_gp_mpc/quadrotor_gp_mpc/gaussian_process.py:158-171.
 * X: dev (N x D), ls: host double[D], K: dev (Np x ldk), ldk >= Np.                  */
GPK_API int gpk_gram(gpk_handle h, int dtype, const void* X, int64_t N, int D, const double* ls,
             double sf2, double diag_add, void* K, int64_t ldk);

/* Row slab of the same matrix, for a Gram build sharded over GPUs by rows (no exchange: rank r writes the rows it
 * owns; the slabs only have to meet on one device if that device is to factorise): Kslab (dev, gpk_padded(nrows) x ldk)
 * receives rows row0 .. row0 + gpk_padded(nrows) - 1 of the padded matrix gpk_gram would write - every entry computed
 * directly (no symmetric mirroring across slabs), diagonal = sf2 + diag_add, identity in the padding.  row0 % 128 == 0.
 * Replaces the same reference lines as gpk_gram.                                                                    */
GPK_API int gpk_gram_rows(gpk_handle h, int dtype, const void* X, int64_t N, int D, const double* ls, double sf2,
                  double diag_add, int64_t row0, int64_t nrows, void* Kslab, int64_t ldk);

/* Cross kernel, transposed layout: B[j][m] = sf2 * exp(-0.5 ||(x_j - xq_m)/ls||^2) for
 * j < N, m < M; zero elsewhere in the (Np x Mp) padded block.  No white noise.
 * Replaces: sklearn/gaussian_process/kernels.py:1564-1565 (cdist + exp).
 * X dev (N x D), Xq dev (M x D), B dev (Np x ldb), ldb >= Mp = gpk_padded(M).          */
GPK_API int gpk_cross_gram_t(gpk_handle h, int dtype, const void* X, int64_t N, const void* Xq,
                     int64_t M, int D, const double* ls, double sf2, void* B, int64_t ldb);

/* ---- K2: blocked Cholesky --------------------------------------------------------
 * In-place lower Cholesky of the padded fp64 matrix A (Np x lda): recursive blocking,
 * 128x128 leaf factorisation in LDS, fp64-MFMA trsm/syrk/gemm tiles.  The strict upper
 * triangle is not referenced and is left as written by gpk_gram.  winv (dev, Np x 128)
 * receives the inverse of every 128x128 diagonal block of L (used by the solves).
 * *info (host) = 0, or the 1-based index of the first non-positive pivot (GPK_NOT_PD).
 * Synchronises.  Replaces: scipy.linalg.cholesky(K, lower=True) at
 * sklearn/gaussian_process/_gpr.py:349,587; gaussian_process.py:184.                  */
GPK_API int gpk_potrf(gpk_handle h, double* A, int64_t Np, int64_t lda, double* winv, int* info);

/* Recompute winv (inverses of the 128x128 diagonal blocks) from an existing padded factor L,
 * e.g. one imported from a scikit-learn pickle (L_ at sklearn/gaussian_process/_gpr.py:349). */
GPK_API int gpk_leaf_inverses(gpk_handle h, const double* L, int64_t Np, int64_t ldl, double* winv);

/* Convert the lower triangle of L and winv to fp32 copies (for the fp32 predict path). */
GPK_API int gpk_factor_to_f32(gpk_handle h, const double* L, int64_t Np, int64_t ldl, const double* winv,
                      float* Lf, int64_t ldlf, float* winvf);

/* ---- K3: alpha = L^-T (L^-1 Y) -----------------------------------------------------
 * Y: dev (N x P) row-major fp64 (already normalised), alpha: dev (N x P).  P <= GPK_MAX_P.
 * Replaces: cho_solve((L, True), y) at sklearn/gaussian_process/_gpr.py:360-364,597;
 * gaussian_process.py:187-189.                                                          */
GPK_API int gpk_potrs(gpk_handle h, const double* L, int64_t Np, int64_t ldl, const double* winv,
              const double* Y, int64_t N, int P, double* alpha);

/* K3 through the explicit inverse factor W = L^-1 (gpk_trtri): alpha = W^T (W Y), two GEMM launches
 * that each stream W once, instead of the 4 Np/128 - 2 launches of the recursive solve.              */
GPK_API int gpk_potrs_inv(gpk_handle h, const double* W, int64_t Np, int64_t ldw, const double* Y, int64_t N,
                  int P, double* alpha);

/* ---- K5 building blocks: B <- L^-1 B, and column sums of squares ---------------------
 * B: dev (Np x ldb) with Mp = multiple of 128 columns in use.  dtype selects fp32/fp64
 * (L, winv and B must all have that dtype).
 * Replaces: solve_triangular(L_, K_trans.T, lower=True) at sklearn/_gpr.py:454-456 and
 * the einsum at :477.                                                                    */
GPK_API int gpk_trsm_lower_left(gpk_handle h, int dtype, const void* L, int64_t Np, int64_t ldl,
                        const void* winv, void* B, int64_t Mp, int64_t ldb);
/* out[m] = sum_{i < Np} B[i][m]^2, accumulated in fp64; out: dev double[Mp].              */
GPK_API int gpk_colsumsq(gpk_handle h, int dtype, const void* B, int64_t Np, int64_t Mp, int64_t ldb,
                 double* out);

/* ---- K4: fused posterior mean -----------------------------------------------------------
 * mean[m][p] = y_mean[p] + y_std[p] * sum_j k(xq_m, x_j) alpha[j][p]; K* is never stored.
 * X dev (N x D), alpha dev (N x P), Xq dev (M x D), mean dev (M x P), all of `dtype`;
 * ls, y_mean, y_std: host double arrays.  D <= GPK_MAX_D_PREDICT, P <= GPK_MAX_P (GPK_BAD_ARG otherwise).
 * Queries must be finite (the host side validates them as scikit-learn does; a NaN coordinate gives k* = 0).
 * Replaces: sklearn/gaussian_process/_gpr.py:441-447 (K_trans @ alpha_, undo normalisation);
 * the 25-call loop at src/px4/mpc.py:1490-1506; gaussian_process.py:223-226.              */
GPK_API int gpk_predict_mean(gpk_handle h, int dtype, const void* X, const void* alpha, int64_t N, int D,
                     int P, const double* ls, double sf2, const double* y_mean,
                     const double* y_std, const void* Xq, int64_t M, void* mean);

/* One-call serving for the control loop (fp64): host queries in, host posterior mean (and variance) out.
 * Copies Xq (host, M x D) through a pinned staging block owned by the handle, runs gpk_predict_mean and -
 * when var_host != NULL - gpk_predict_var_inv with the explicit inverse factor W (dev Np x ldw, gpk_trtri),
 * copies the results back and synchronises the handle's stream: one call and one synchronisation per MPC
 * step instead of an upload, two launch chains and two downloads driven from the host language.
 * mean_host: M x P (un-normalised with y_mean / y_std); var_host: M (normalised-target units: the caller
 * scales by y_std^2), clipped below at floor_.  1 <= M <= GPK_HOST_MAX_M.
 * Replaces: the per-call path of src/px4/simple_gp.py:187-201 (predict_residual) and the 25-call loop of
 * src/px4/mpc.py:1490-1506; sklearn/_gpr.py:441-494.
 * Up to 32 queries (D, P <= 16, N <= 16384) take two dedicated launches (K* + mean shares; 16 rows of W per
 * workgroup on the fp64 MFMA, last-workgroup reductions) instead of the general chain's seven.           */
#define GPK_HOST_MAX_M 4096
GPK_API int gpk_predict_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P,
                     const double* ls, double sf2, const double* y_mean, const double* y_std,
                     const double* W, int64_t Np, int64_t ldw, double kss, double floor_,
                     const double* Xq_host, int64_t M, double* mean_host, double* var_host);

/* The same one-call serving for B <= 8 single-output models that share the query batch - the per-axis GPs of
 * gp_trainer.py / pretrained_gp.py - in ONE call and two launches (model = second grid dimension).
 * X, alpha, W: arrays of B device pointers (N x D, N x 1, Np x ldw); ls: B x D (host); sf2, y_mean, y_std, kss:
 * B (host).  1 <= M <= 32, D <= 16, N <= 16384.  mean_host: B x M (un-normalised); var_host: B x M in
 * normalised-target units, or NULL (then W and kss may be NULL).
 * Replaces: the loop over six scalar GPs of src/px4/pretrained_gp.py:52-98.                                 */
GPK_API int gpk_predict_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                           const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                           const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                           const double* Xq_host, int64_t M, double* mean_host, double* var_host);

/* K4 on the matrix cores, fp32 only: the same posterior mean as gpk_predict_mean(GPK_F32, ...), with the
 * pairwise squared distances of 32 x 32 (query, training point) blocks formed by MFMAs from centred, scaled
 * coordinates (|a|^2 + |b|^2 - 2 a.b as ONE augmented dot product of depth D + 2) and only exp2 + P FMAs per
 * pair left on the vector ALU.  D <= 14: six v_mfma_f32_32x32x16_bf16 per block on an exact three-way bf16
 * split of every fp32 operand (fp32-accurate distances); the training side is centred, scaled and split once
 * per call into MFMA-fragment order (N x 96 bytes of the handle's scratch) and loaded from L2 straight into
 * registers.  D = 15, 16: nine v_mfma_f32_32x32x2_f32.  The training set is cut into chunks of <= 2048
 * points whose partial sums are added in fp64.  center: host double[D], a point near the data (the
 * training mean); the expansion is accurate to ~|u|^2 * 2^-23 in the exponent, u = (x - center) / ls, so
 * callers use it while max |u|^2 is modest (device.py: <= 64) and the exact-difference kernel otherwise.
 * D <= 16, P <= 8.  Replaces the same reference lines as gpk_predict_mean.                              */
GPK_API int gpk_predict_mean_mfma(gpk_handle h, const float* X, const float* alpha, int64_t N, int D, int P,
                          const double* ls, double sf2, const double* center, const double* y_mean,
                          const double* y_std, const float* Xq, int64_t M, float* mean);

/* K5 on the bf16 matrix pipe at fp32 accuracy (exact operand split).
 * gpk_split3: src (dev rows x ld fp32, cols % 16 == 0) -> dst (dev, rows * cols * 6 bytes): every fp32 value
 * as three bf16 parts x = x0 + x1 + x2 (8 significant bits each, rounded to nearest: the sum is exact), stored as
 * 16-byte chunks [row / 4][k16 block][row % 4][half][part] (rows % 4 == 0; 96 bytes per row and 16 columns).
 * gpk_predict_var_inv_split: the same result as gpk_predict_var_inv(GPK_F32, ...) with W3 = gpk_split3 of the
 * fp32 inverse factor (gpk_tril_to_f32 output, Np x Np): one launch whose 32 x 32 x 16 block products are six
 * v_mfma_f32_32x32x16_bf16 each (a0 b0, a0 b1, a1 b0, a1 b1, a0 b2, a2 b0; exact bf16 products, fp32
 * accumulation; the dropped terms are below 2^-24 of |a||b|).  work: dev float[Mp * Np] (K* in fp32),
 * work3: dev, Mp * Np * 6 bytes (its split); var: dev double[Mp].  X, Xq fp32.
 * Replaces the same reference lines as gpk_predict_var (sklearn/gaussian_process/_gpr.py:454-485).       */
GPK_API int gpk_split3(gpk_handle h, const float* src, int64_t rows, int64_t cols, int64_t ld, void* dst);
GPK_API int gpk_predict_var_inv_split(gpk_handle h, const float* X, int64_t N, int D, const double* ls, double sf2,
                              const void* W3, int64_t Np, const float* Xq, int64_t M, double kss, double floor_,
                              float* work, void* work3, double* var);

/* The same launch with an fp16 x 2 operand split, three products per block, both operands in "fragment order" and one
 * scale per 128-row block of W (the fp32 serving default of the Python host side and of gpk_predict).
 * gpk_split2_rows: W (dev n x ld fp32 inverse factor, gpk_tril_to_f32 output, n % 128 == 0) -> scales (dev float[n / 128]:
 * for each 128-row block the largest power of two s with s * max |W_ij| <= 2^15, the maximum taken over the block's part of
 * the lower triangle - computed on the device, no synchronisation) and dst (dev, n * n * 4 bytes): x s = h0 + h1 + r with
 * h0, h1 fp16 rounded to nearest, |r| <= max(2^-23 |x s|, 2^-25) (relative for entries within 2^-17 of 2^15, absolute
 * below that, where h1 is a subnormal fp16); 16-byte chunks in fragment order: chunk (row, k16 block kb,
 * k half h, part p) at index (((row / 32) * (n / 16) + kb) * 2 + p) * 64 + h * 32 + row % 32 - the 64 chunks of one
 * v_mfma_f32_32x32x16_f16 operand are 1 KiB of contiguous memory.
 * gpk_predict_var_inv_split2: the result of gpk_predict_var_inv(GPK_F32, ...) from W2 / w_scales = gpk_split2_rows of the
 * fp32 inverse factor: K* (scaled by the power of two below 2^15 / sf2) is computed straight into the same layout
 * (work2: dev, Mp * Np * 4 bytes; no fp32 panel exists), and ONE launch forms V = W K*^T on the fp16 matrix pipe - block
 * products a1 b0 + a0 b1 + a0 b0 on v_mfma_f32_32x32x16_f16, fp32 accumulation: half the matrix-pipe work of the bf16 x 3
 * split - with every operand fragment loaded from L2 straight into registers (no LDS), reduced to column sums of squares
 * in its epilogue.  With round-to-nearest parts a0 + a1 reproduces a to 2^-23 at worst and the dropped a1 b1 is below
 * 2^-22 |a b|; measured over 31 random models the error of |W k*|^2 equals that of the exact-fp32 MFMA launch
 * (profiles/r02_fp32_variance_forms_accuracy.log).  var: dev double[Mp].  D <= 16.
 * Replaces the same reference lines as gpk_predict_var (sklearn/gaussian_process/_gpr.py:454-485).                  */
GPK_API int gpk_split2_rows(gpk_handle h, const float* W, int64_t n, int64_t ld, float* scales, void* dst);
/* gpk_split2_rows_f64: the same scales and parts straight from the fp64 inverse factor (gpk_trtri output, dev n x ld doubles):
 * every entry is rounded to fp32 on the fly exactly as gpk_tril_to_f32 would have stored it, so the result is bit-identical
 * on the lower tiles while the fp32 copy (17 GB at N = 65 536) and two passes over it are gone; the 16-column blocks right of
 * a row's diagonal tile - which the variance launch never reads - are left unwritten.                                    */
GPK_API int gpk_split2_rows_f64(gpk_handle h, const double* W, int64_t n, int64_t ld, float* scales, void* dst);
/* gpk_split2_rows_f64_absmax: the same with the first pass over W done already: on entry scales[n / 128] holds max |(float)W_ij|
 * over the lower triangle of each 128-row block - what gpk_trtri_absmax leaves behind - and the call turns it into the scales
 * and writes the parts: ONE pass over W (read 8, write 4 bytes per lower-tile entry) instead of two.  Same bits.             */
GPK_API int gpk_split2_rows_f64_absmax(gpk_handle h, const double* W, int64_t n, int64_t ld, float* scales, void* dst);
GPK_API int gpk_predict_var_inv_split2(gpk_handle h, const float* X, int64_t N, int D, const double* ls, double sf2,
                                       const void* W2, const float* w_scales, int64_t Np, const float* Xq, int64_t M,
                                       double kss, double floor_, void* work2, double* var);

/* One fp32 serving step in one call, the whole result in one buffer: out (dev double, M x 2P) row m =
 * [mean[m][0..P) | var[m] y_std[p]^2, p = 0..P) - K4 (gpk_predict_mean_mfma when `center` is given, else
 * gpk_predict_mean(GPK_F32)) into mean_tmp (dev float[M * P]), then gpk_predict_var_inv_split2's launch with the variance's
 * un-normalisation (sklearn/gaussian_process/_gpr.py:487-489) and the packing folded into its finalising kernel; that
 * kernel also adds to *low_count (dev, nullable; a running counter: the caller reads it before and after, or zeroes
 * it) the number of rows whose normalised variance is below `recheck_below` - the rows the fp32 serving gate
 * recomputes in fp64.
 * gpk_pack_mean_var: the same rows from a separate mean (dev M x P of `dtype`) and normalised variance (dev double[M]) -
 * for the serving paths whose variance comes from another launch.  P <= 16.                                          */
GPK_API int gpk_predict_mean_var_split2(gpk_handle h, const float* X, const float* alpha, int64_t N, int D, int P,
                                        const double* ls, double sf2, const double* center, const double* y_mean,
                                        const double* y_std, const void* W2, const float* w_scales, int64_t Np,
                                        const float* Xq, int64_t M, double kss, double floor_, void* work2,
                                        float* mean_tmp, double recheck_below, unsigned* low_count, double* out);
GPK_API int gpk_pack_mean_var(gpk_handle h, int dtype, const void* mean, const double* var, int64_t M, int P,
                              const double* y_std, double* out);

/* K4 for B (<= 8) independent single-output ARD models that share X (the per-axis GPs of
 * src/px4/gp_trainer.py:139-179, predicted one by one at src/px4/pretrained_gp.py:64-91): one launch
 * evaluates every model; the feature differences of a (query, training point) pair are formed once.
 * alpha: dev (N x B), column b = model b; ls: host double[B*D] (row b = model b's ARD length-scales);
 * sf2, y_mean, y_std: host double[B]; mean: dev (M x B).  X, alpha, Xq, mean of `dtype`.  D <= 16.      */
GPK_API int gpk_predict_mean_multi(gpk_handle h, int dtype, const void* X, const void* alpha, int64_t N, int D,
                           int B, const double* ls, const double* sf2, const double* y_mean,
                           const double* y_std, const void* Xq, int64_t M, void* mean);

/* ---- K5: posterior variance ---------------------------------------------------------------
 * var[m] = max(kss - sum_i (L^-1 k*_m)_i^2, floor) in units of the normalised targets
 * (caller multiplies by y_std^2).  kss = sf2 (+ noise for the sklearn surface).
 * work: dev scratch of at least Np * Mp elements of `dtype` (Mp = gpk_padded(M)).
 * var: dev double[Mp] (only the first M entries are meaningful).
 * Replaces: sklearn/gaussian_process/_gpr.py:454-485; gaussian_process.py:229-232.          */
GPK_API int gpk_predict_var(gpk_handle h, int dtype, const void* X, int64_t N, int D, const double* ls,
                    double sf2, const void* L, int64_t Np, int64_t ldl, const void* winv,
                    const void* Xq, int64_t M, double kss, double floor, void* work,
                    double* var);

/* ---- K5, serving form: variance through the explicit inverse factor ---------------------------------
 * gpk_trtri: W (dev Np x ldw, fp64) <- L^-1, lower triangle by tiles (recursive, fp64-MFMA GEMMs);
 * one-off N^3/3 flops after the factorisation.  work: dev double[(Np/2 + 128)^2].  Besides the lower
 * triangle it writes zeros into the 15 tiles to the right of every diagonal tile (see below).
 * gpk_tril_to_f32: fp32 copy of the lower triangle, with the same band of zeros right of the diagonal.
 * gpk_predict_var_inv: var[m] = max(kss - |W k*_m|^2, floor) in ONE GEMM launch: the tile of
 * V = W K*^T is reduced to column sums of squares in the epilogue and never written to HBM; W's
 * zero upper triangle is skipped (N^2 M flops, + 1.4 %: the tile rows of a super-tile all run to the
 * end of the longest row so that its 64 workgroups stay in lockstep and share operand panels through L2 -
 * W must therefore be ZERO above the diagonal for 16 tiles (2048 columns) from each row's diagonal tile
 * rightwards, which gpk_trtri and gpk_tril_to_f32 guarantee).  W, X, Xq of `dtype`; work: dev scratch
 * of Mp * Np elements of `dtype`; var: dev double[M] (only M entries are written).
 * Replaces the same reference lines as gpk_predict_var (sklearn/gaussian_process/_gpr.py:454-485),
 * with solve_triangular(L, K*^T) evaluated as (L^-1) K*^T.                                          */
GPK_API int gpk_trtri(gpk_handle h, const double* L, int64_t Np, int64_t ldl, const double* winv, double* W,
              int64_t ldw, double* work);
/* gpk_trtri_absmax: gpk_trtri that also leaves block_absmax[Np / 128] (dev) = max |(float)W_ij| over the lower triangle of each
 * 128-row block, accumulated as the tiles of W are written (the epilogue of the level products; no pass over W): the first
 * half of gpk_split2_rows_f64, for gpk_split2_rows_f64_absmax.  Not in batched mode.                                        */
GPK_API int gpk_trtri_absmax(gpk_handle h, const double* L, int64_t Np, int64_t ldl, const double* winv, double* W,
              int64_t ldw, double* work, float* block_absmax);
GPK_API int gpk_tril_to_f32(gpk_handle h, const double* A, int64_t Np, int64_t lda, float* Af, int64_t ldaf);
GPK_API int gpk_predict_var_inv(gpk_handle h, int dtype, const void* X, int64_t N, int D, const double* ls,
                        double sf2, const void* W, int64_t Np, int64_t ldw, const void* Xq, int64_t M,
                        double kss, double floor, void* work, double* var);

/* ---- K7: posterior covariance --------------------------------------------------------------------------------------
 * cov (dev, Mp x ldc fp64, Mp = gpk_padded(M), ldc >= Mp) <- K(Xq, Xq) + noise I - V^T V, V = L^-1 K*^T, in units of the
 * normalised targets (the caller scales output p by y_std[p]^2) and never clipped.  K(Xq, Xq) by exact differences of the
 * queries divided by the length-scales; noise (the WhiteKernel level) only where the row index equals the column index, as
 * WhiteKernel's k(X) does - never on duplicate rows.  Rows / columns >= M of the padded block are 0.  Symmetric bit for bit:
 * ONE tile GEMM over the lower 128 x 128 tiles whose epilogue stores every tile and its transpose (diagonal tiles: the lower
 * half, mirrored).  work: dev double[Np * Mp] (V); the handle's scratch holds the rest.  fp64 only (dtype = GPK_F64), D <= 16.
 * gpk_predict_cov_inv: V = W K*^T with the explicit inverse factor W (dev Np x ldw, gpk_trtri): N^2 M + N M^2 flops.
 * gpk_predict_cov: V by the blocked triangular solve with L and winv (gpk_potrf) - for models whose inverse factor is not formed.
 * Replaces: sklearn/gaussian_process/_gpr.py:454-464 (solve_triangular, kernel_(X) - V.T @ V).                              */
GPK_API int gpk_predict_cov_inv(gpk_handle h, int dtype, const void* X, int64_t N, int D, const double* ls, double sf2,
                                const void* W, int64_t Np, int64_t ldw, const void* Xq, int64_t M, double noise, void* work,
                                double* cov, int64_t ldc);
GPK_API int gpk_predict_cov(gpk_handle h, int dtype, const void* X, int64_t N, int D, const double* ls, double sf2,
                            const void* L, int64_t Np, int64_t ldl, const void* winv, const void* Xq, int64_t M, double noise,
                            void* work, double* cov, int64_t ldc);
/* One-call mean + covariance for small batches (fp64), the covariance analogue of gpk_predict_host: host queries in
 * (M x D), host mean (M x P, un-normalised) and cov (M x M, normalised-target units) out, one synchronisation.  W: the
 * inverse factor (dev Np x ldw).  Up to 32 queries (D, P <= 16, N <= 16384): two launches - small_cross_mean_kernel and
 * small_cov_kernel (16 rows of W per workgroup on the fp64 MFMA, each workgroup's 32 x 32 share of V^T V added in a fixed
 * two-level order: bit-identical from run to run, no floating-point atomics); 33 .. GPK_HOST_MAX_M queries: the fused mean
 * and gpk_predict_cov_inv inside the same call.
 * Replaces: sklearn/gaussian_process/_gpr.py:441-469 (predict(X, return_cov=True) before the un-normalisation of the
 * covariance) for the GP-MPC horizon of src/px4/mpc.py:1490-1506.                                                           */
GPK_API int gpk_predict_host_cov(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P,
                                 const double* ls, double sf2, const double* y_mean, const double* y_std, const double* W,
                                 int64_t Np, int64_t ldw, double noise, const double* Xq_host, int64_t M, double* mean_host,
                                 double* cov_host);
/* K7 for B (<= 8) single-output ARD models on one query batch - the per-axis layout of src/px4/gp_trainer.py:139-179: the joint
 * posterior of every model over the same rows (a consistent residual trajectory per axis along the horizon).
 * gpk_predict_host_multi_cov: the one-call serving form, arguments and limits as gpk_predict_host_multi_grad (X / alpha / W:
 *   host arrays of B device pointers; ls host B x D; sf2, y_mean, y_std host double[B]), 1 <= M <= 32, D <= 16, N <= 16384.
 *   noise host double[B]: model b's WhiteKernel level, added only where row = column.  mean_host (B x M) un-normalised;
 *   cov_host (B x M x M) in normalised-target units, not clipped.  The two launches of gpk_predict_host_cov with the model as a
 *   grid dimension: all B covariances in TWO launches and one synchronisation, queries and results through the pinned, mapped
 *   block; every model has its own shares, group sums and ticket counters and the order of every sum depends on Np and M
 *   only: model b's block has the bits of gpk_predict_host_cov on that model alone, symmetric bit for bit, the same from run
 *   to run.  With option small_path = 0: the general building blocks (fused mean, gpk_predict_cov_inv), model by model, one
 *   strided download each (a cross-check).
 *   Replaces: six times sklearn/gaussian_process/_gpr.py:441-469 (predict(X, return_cov=True)) around the per-axis loop of
 *   src/px4/pretrained_gp.py:52-98; within this library, B gpk_predict_host_cov calls with 2 B launches and B synchronisations.
 * gpk_predict_batched_cov: the composite on the object of gpk_fit_batched, host fp64 buffers: Xq (M x D), mean (M x B), cov
 *   (B x M x M) in target units (already multiplied by y_std[b]^2), model b's own noise level on its diagonal.  Up to 32
 *   queries (N <= 16384): one gpk_predict_host_multi_cov; larger batches (M <= 16384): gpk_predict_mean_multi and one
 *   gpk_predict_cov_inv per model, one synchronisation.  Checks that the queries are finite.                              */
GPK_API int gpk_predict_host_multi_cov(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                       int D, const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                       const double* const* W, int64_t Np, int64_t ldw, const double* noise,
                                       const double* Xq_host, int64_t M, double* mean_host, double* cov_host);
GPK_API int gpk_predict_batched_cov(gpk_handle h, const double* Xq, int64_t M, double* mean, double* cov);

/* ---- K8: input gradients of the posterior (fp64) ------------------------------------------------------------------
 * With u_jd = (x_jd - xq_md) / ls_d^2 (exact differences):
 *   dmean[m][p][d] = y_std[p] sum_j k(xq_m, x_j) u_jd alpha[j][p]                  (un-normalised, like gpk_predict_mean)
 *   dvar[m][d]     = -2 sum_j k(xq_m, x_j) u_jd c_j,   c = K^-1 k* = W^T (W k*)    (normalised-target units)
 * The N x M x D tensor of kernel derivatives is never stored.  dvar is the gradient of the UNCLIPPED kss - |W k*|^2; var is
 * clipped exactly as gpk_predict_var_inv clips it.  The gradient of the standard deviation is dvar / (2 std).
 * gpk_predict_mean_grad: one fused launch in the tiling of gpk_predict_mean (training rows through LDS, one exp per pair,
 *   D x P running sums per query split into output groups of <= 4) + the fixed-order reduction of the training chunks.
 *   X dev (N x D), alpha dev (N x P), Xq dev (M x D), dmean dev (M x P x D); ls, y_std host.  D, P <= 16.
 * gpk_predict_var_grad_inv: K* (gpk_cross_gram_t), V = W K* and C = W^T V (two tile GEMMs on the fp64 matrix cores, W's zero
 *   triangle skipped in both: 2 N^2 M flops), then ONE streaming pass over the three Np x Mp panels.  W: the inverse factor
 *   (dev Np x ldw, gpk_trtri); work: dev double[3 * Np * Mp], Mp = gpk_padded(M); var: dev double[M] or NULL; dvar: dev (M x D).
 *   Queries are independent: a caller panels them as it likes (there is no solve route and no fp32 form).
 * gpk_predict_host_grad: the one-call serving form - host queries in (M x D), host results out, one synchronisation, queries
 *   and results through the handle's pinned, mapped block.  mean_host (M x P) and dmean_host (M x P x D) un-normalised;
 *   var_host (M) and dvar_host (M x D) in normalised-target units, or both NULL: mean + Jacobian only (W may then be NULL).
 *   Up to 32 queries (D, P <= 16, N <= 16384): mean + Jacobian in ONE launch (the Jacobian's shares ride in
 *   small_cross_mean_kernel), all four results in three (+ small_var_kernel storing V, + small_wtv_grad_kernel), every
 *   reduction by the last workgroup in a fixed order: bit-identical from run to run.  33 .. GPK_HOST_MAX_M queries: the two
 *   building blocks above inside the same call, the variance gradient in query panels of <= 6 GiB.
 * gpk_predict_model_grad: the composite - the model of gpk_fit / gpk_import, host fp64 buffers: Xq (M x D), mean (M x P),
 *   dmean (M x P x D), and var (M x P) / dvar (M x P x D) per output (already multiplied by y_std[p]^2), or both NULL;
 *   var_includes_noise as in gpk_predict.  Forms the inverse factor if the model does not hold it yet.  Any M.
 * Replaces: nothing in the reference - scikit-learn has no gradient call.  A caller would take central differences of
 *   GaussianProcessRegressor.predict (sklearn/gaussian_process/_gpr.py:441-494), 2 D (fourth order: 4 D) calls per horizon,
 *   around the loop of src/px4/mpc.py:1490-1506; the consumer is the linearisation of
 *   quadrotor_gp_mpc/quadrotor_gp_mpc/mpc_controller.py:318 (linearize_dynamics).                                          */
GPK_API int gpk_predict_mean_grad(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                  double sf2, const double* y_std, const double* Xq, int64_t M, double* dmean);
GPK_API int gpk_predict_var_grad_inv(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2,
                                     const double* W, int64_t Np, int64_t ldw, const double* Xq, int64_t M, double kss,
                                     double floor, double* work, double* var, double* dvar);
GPK_API int gpk_predict_host_grad(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                  double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np,
                                  int64_t ldw, double kss, double floor, const double* Xq_host, int64_t M, double* mean_host,
                                  double* var_host, double* dmean_host, double* dvar_host);
GPK_API int gpk_predict_model_grad(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var, double* dmean,
                                   double* dvar, int var_includes_noise);
/* K8 for B (<= 8) single-output ARD models on one query batch - the per-axis layout of src/px4/gp_trainer.py:139-179 as
 * gpk_predict_host_multi / gpk_predict_mean_multi serve it; formulas and units as above, model by model.
 * gpk_predict_host_multi_grad: the one-call serving form, arguments as gpk_predict_host_multi (X / alpha / W: host arrays of B
 *   device pointers; ls host B x D; sf2, y_mean, y_std, kss host double[B]), 1 <= M <= 32, D <= 16, N <= 16384.  mean_host
 *   (B x M) and dmean_host (B x M x D) un-normalised; var_host (B x M) and dvar_host (B x M x D) in normalised-target units,
 *   or both NULL (W and kss may then be NULL too).  The three gradient launches of gpk_predict_host_grad with the model as a
 *   grid dimension: mean + Jacobian of ALL models in ONE launch, all four results in THREE, one synchronisation, queries and
 *   results through the pinned, mapped block; every model has its own shares and ticket counters, every reduction is done by
 *   the last workgroup in a fixed order (no floating-point atomics): bit-identical from run to run, and for B = 1 the bits of
 *   gpk_predict_host_grad.  With option small_path = 0: the general building blocks, model by model (a cross-check).
 *   Replaces: nothing in the reference, which has no gradient call - a caller of PreTrainedGP.predict_residual
 *   (src/px4/pretrained_gp.py:52-98) would take central differences, 4 D calls of six scikit-learn predictions each; within
 *   this library, B gpk_predict_host_grad calls with B synchronisations.
 * gpk_predict_mean_grad_multi: the Jacobian companion of gpk_predict_mean_multi for any M, all device pointers: X (N x D),
 *   alpha (N x B, column b = model b), Xq (M x D), dmean (M x B x D); ls host (B x D); sf2, y_std host double[B].  One fused
 *   launch: the raw feature differences of a (query, training point) pair are formed once and serve every model's distance
 *   and every model's D gradient sums; models in groups of <= 4 over the third grid dimension (<= 64 fp64 accumulators per
 *   thread, no scratch); the training chunks are added in chunk order.
 *   Replaces: B gpk_predict_mean_grad launches (the differences formed B times); in the reference, as above.
 * gpk_predict_batched_grad: the composite on the object of gpk_fit_batched, host fp64 buffers: Xq (M x D), mean (M x B),
 *   dmean (M x B x D), and var (M x B) / dvar (M x B x D) in target units (already multiplied by y_std[b]^2), or both NULL;
 *   var_includes_noise as in gpk_predict.  Up to 32 queries (N <= 16384): gpk_predict_host_multi_grad; larger batches in
 *   panels: gpk_predict_mean_multi + gpk_predict_mean_grad_multi and one gpk_predict_var_grad_inv per model.  Any M.
 *   Replaces: central differences around PreTrainedGP.predict_residual's loop, src/px4/pretrained_gp.py:52-98.          */
GPK_API int gpk_predict_host_multi_grad(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                        int D, const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                        const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor,
                                        const double* Xq_host, int64_t M, double* mean_host, double* var_host,
                                        double* dmean_host, double* dvar_host);
GPK_API int gpk_predict_mean_grad_multi(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int B,
                                        const double* ls, const double* sf2, const double* y_std, const double* Xq, int64_t M,
                                        double* dmean);
GPK_API int gpk_predict_batched_grad(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var, double* dmean,
                                     double* dvar, int var_includes_noise);

/* ---- K8, second derivatives: the input Hessian of the posterior mean (fp64) -----------------------------------------------
 * With q = xq_m / ls, r_j = x_j / ls, delta_j = q - r_j (exact differences, formed before any product) and
 * k_j = sf2 exp(-|delta_j|^2 / 2) (no White term):
 *   T_p[d][e] = sum_j k_j alpha[j][p] delta_jd delta_je,   S_p = sum_j k_j alpha[j][p]
 *   hess[m][p][d][e] = y_std[p] / (ls_d ls_e) (T_p[d][e] - [d = e] S_p)            (un-normalised, the units of dmean)
 * hess holds the full D x D block per (query, output); both triangles are written from ONE sum: hess[m][p][d][e] and
 * hess[m][p][e][d] have the same bits.  A null hess is GPK_BAD_ARG; every refusal happens before any launch.
 * gpk_predict_mean_hess: one fused launch in the tiling of gpk_predict_mean_grad (training rows through LDS already divided
 *   by ls, one exp per pair) + the fixed-order reduction of the training chunks (no floating-point atomics: bit-identical from
 *   run to run).  The D (D + 1) / 2 + 1 running sums per (query, output) are split over the third grid dimension into output
 *   groups and blocks of whole rows of the triangle (<= 64 fp64 accumulators per thread, no scratch); a group recomputes the
 *   pair's kernel value.  The chunks' partial sums stay within 256 MiB: fewer chunks, then smaller query panels.
 *   X dev (N x D), alpha dev (N x P), Xq dev (M x D), hess dev (M x P x D x D); ls, y_std host.  D, P <= 16, any M.
 * gpk_predict_host_hess: the one-call serving form, arguments as gpk_predict_host_grad without the variance ones: host
 *   queries in (M x D), mean_host (M x P), dmean_host (M x P x D) and hess_host (M x P x D x D) out, one synchronisation,
 *   queries and results through the handle's pinned, mapped block.  1 <= M <= GPK_HOST_MAX_M.  mean and dmean come from the
 *   launches of gpk_predict_host_grad and have its bits.  Up to 32 queries (D, P <= 16, N <= 16384): TWO launches and no copy
 *   command - small_cross_mean_jac_kernel, untouched, then small_hess_kernel: a workgroup forms the share of T and S of its
 *   max(32, Np / 64) training rows for a slice of about 512 entries, the last workgroup of every slice (its own ticket, left
 *   at zero) adds that slice of the shares in workgroup order and writes the Hessians straight into the pinned block; the
 *   grouping depends on (Np, M, P, D) alone.  33 .. GPK_HOST_MAX_M queries, and option small_path = 0 (the cross-check): one
 *   query upload and the general blocks gpk_predict_mean, gpk_predict_mean_grad, gpk_predict_mean_hess (6 launches).
 * gpk_predict_host_multi_hess: B (<= 8) single-output ARD models on one query batch, arguments and limits as
 *   gpk_predict_host_multi_grad without the variance ones; mean_host (B x M), dmean_host (B x M x D), hess_host
 *   (B x M x D x D).  The two launches of gpk_predict_host_hess with the model as a grid dimension - TWO launches and one
 *   synchronisation for all models, every model with its own shares and tickets: block b has the bits of model b served alone
 *   (B = 1: the bits of gpk_predict_host_hess).  Option small_path = 0: the general blocks, model by model (a cross-check).
 * gpk_predict_model_hess: the composite on the model of gpk_fit / gpk_import, host fp64 buffers: Xq (M x D), mean (M x P),
 *   dmean (M x P x D), hess (M x P x D x D).  Any M (query blocks whose Hessians stay within 32 MiB of pinned memory).
 * Replaces: nothing in the reference - scikit-learn has no derivative call.  A caller would difference
 *   GaussianProcessRegressor.predict (sklearn/gaussian_process/_gpr.py:441-494) twice; within this library, 2 D (fourth
 *   order: 4 D) gpk_predict_host_grad calls, each with its own synchronisation.                                            */
GPK_API int gpk_predict_mean_hess(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                  double sf2, const double* y_std, const double* Xq, int64_t M, double* hess);
GPK_API int gpk_predict_host_hess(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                  double sf2, const double* y_mean, const double* y_std, const double* Xq_host, int64_t M,
                                  double* mean_host, double* dmean_host, double* hess_host);
GPK_API int gpk_predict_host_multi_hess(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                        int D, const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                        const double* Xq_host, int64_t M, double* mean_host, double* dmean_host,
                                        double* hess_host);
GPK_API int gpk_predict_model_hess(gpk_handle h, const double* Xq, int64_t M, double* mean, double* dmean, double* hess);
/* gpk_predict_mean_hess_multi: the Hessian companion of gpk_predict_mean_grad_multi for B (<= 8) single-output ARD models on
 *   shared inputs, any M, arguments as that entry: X (N x D), alpha (N x B, column b = model b), Xq (M x D) dev; ls host (B x D);
 *   sf2, y_std host double[B]; hess dev (M x B x D x D).  One fused launch: the raw feature differences of a pair and each
 *   product of two of them are formed once and serve every model's distance and every model's sums (1 / ls^2 weights in LDS,
 *   the factor 1 / (ls_bd ls_be) applied by the reduction); the models in groups of two (D <= 4: up to four) and the triangle in
 *   blocks of whole rows over the third grid dimension (<= 64 fp64 accumulators, no scratch); the training chunks added in
 *   chunk order, both triangles written from one sum.  One launch pair instead of B - but measured SLOWER than B
 *   gpk_predict_mean_hess launches at M = 4096 (B = 6, D = 10: 0.90 x at N = 4096, 0.83 x at N = 16384; D = 16: 0.60 x;
 *   DESIGN.md, K8, second derivatives): every (model group, row block) recomputes the models' distances and exp.
 * gpk_predict_batched_hess: the composite on the object of gpk_fit_batched, host fp64 buffers: Xq (M x D), mean (M x B), dmean
 *   (M x B x D), hess (M x B x D x D).  Up to 32 queries (N <= 16384): gpk_predict_host_multi_hess; larger batches in panels:
 *   gpk_predict_mean_multi + gpk_predict_mean_grad_multi (the bits of gpk_predict_batched_grad) and
 *   gpk_predict_mean_hess_multi.  Any M.                                                                                   */
GPK_API int gpk_predict_mean_hess_multi(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int B,
                                        const double* ls, const double* sf2, const double* y_std, const double* Xq, int64_t M,
                                        double* hess);
GPK_API int gpk_predict_batched_hess(gpk_handle h, const double* Xq, int64_t M, double* mean, double* dmean, double* hess);

/* ---- K6a: log-marginal-likelihood terms -----------------------------------------------------
 * terms[0] = sum_{i<N} log L[i][i]; terms[1 + p] = sum_i Y[i][p] * alpha[i][p]  (host doubles).
 * Synchronises.  Replaces: sklearn/gaussian_process/_gpr.py:609-613; gaussian_process.py:250-261. */
GPK_API int gpk_lml_terms(gpk_handle h, const double* L, int64_t N, int64_t ldl, const double* Y,
                  const double* alpha, int P, double* terms);

/* ---- K6b: K^-1 and the fused LML-gradient reduction --------------------------------------------
 * gpk_potri: Kinv (dev Np x ldk) <- lower triangle of (L L^T)^-1 (trtri + W^T W on fp64 MFMA).
 * L is not modified.  work: dev double[Np * Np].
 * Replaces: cho_solve((L, True), eye(N)) at sklearn/gaussian_process/_gpr.py:627-629.           */
GPK_API int gpk_potri(gpk_handle h, const double* L, int64_t Np, int64_t ldl, const double* winv,
              double* Kinv, int64_t ldk, double* work);
/* The second half of gpk_potri when W = L^-1 is already at hand: Kinv (lower tiles) = W^T W.       */
GPK_API int gpk_wtw(gpk_handle h, const double* W, int64_t Np, int64_t ldw, double* Kinv, int64_t ldk);
/* grad[d] (d < D) = 0.5 * sum_ij Q_ij K_ij ((x_id - x_jd)/ls_d)^2, grad[D] = 0.5 * noise * tr(Q),
 * Q = alpha alpha^T - P * Kinv, K_ij = sf2 exp(-0.5 d2_ij) recomputed on the fly (the
 * N x N x D tensor sklearn builds at kernels.py:1576-1579 is never materialised).
 * grad: host double[D + 2] = [g_ls_0 .. g_ls_{D-1}, g_noise, g_sf2] with g_sf2 = 0.5 * sum_ij Q_ij K_ij
 * (the signal-variance gradient used by the package GP).  D <= 16.  Synchronises.
 * Replaces: sklearn/gaussian_process/_gpr.py:615-647 + sklearn/gaussian_process/kernels.py:1571-1580,
 * :1403-1408.                                                                                     */
GPK_API int gpk_lml_grad(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2,
                 double noise, const double* alpha, int P, const double* Kinv, int64_t ldk,
                 double* grad);

/* Kernel matrix of two point sets and its length-scale derivative factor, as the package GP's kernel OBJECT hands them out:
 * K[i][j] = sf2 exp(-r2_ij / 2), Q[i][j] = K[i][j] r2_ij, r2_ij = sum_d ((x1_id - x2_jd) / ls_d)^2 by exact differences
 * (the reference's norm expansion, gaussian_process.py:38, differs by ~3e-14 on the flight data).  For its isotropic kernel
 * dK/dl = Q / l and dK/dsf2 = K / sf2.  X1 dev (n1 x D), X2 dev (n2 x D), K and Q (Q may be NULL) dev (n1 x ld), ld >= n2, no
 * padding; D <= 16.  Asynchronous on the handle's stream.
 * Replaces: RBFKernel.__call__ / RBFKernel.gradient / GaussianProcess.compute_kernel_matrix,
 * quadrotor_gp_mpc/quadrotor_gp_mpc/gaussian_process.py:26-60,158-171.                                              */
GPK_API int gpk_rbf_kernel_grad(gpk_handle h, const double* X1, int64_t n1, const double* X2, int64_t n2, int D,
                        const double* ls, double sf2, double* K, double* Q, int64_t ld);

/* ---- one optimiser evaluation as one chain ------------------------------------------------------------------------
 * gpk_lml_eval: K1 (Gram of X with ls, sf2, diag_add = noise + jitter, into K), K2 (factor in place, winv), W = L^-1 (work:
 * the scratch of gpk_trtri), alpha = W^T (W Yn), the terms of gpk_lml_terms and - grad != NULL - K^-1 = W^T W (Kinv) and the
 * gradient of gpk_lml_grad: the same launches as the call-by-call route, queued back to back with ONE synchronisation
 * (call by call there are three: the pivot check, the terms, the gradient).  Device pointers except ls, terms[1 + P],
 * grad[D + 2], info (host).  Returns GPK_NOT_PD with *info as gpk_potrf (terms / grad then hold nothing).  Np = gpk_padded(N).
 * Replaces: one call of log_marginal_likelihood(theta, eval_gradient=True), sklearn/gaussian_process/_gpr.py:537-652, as the
 * optimiser of GaussianProcessRegressor.fit makes it (src/px4/simple_gp.py:167-177).                                      */
GPK_API int gpk_lml_eval(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2, double diag_add,
                 double noise, const double* Yn, int P, double* K, int64_t Np, double* winv, double* W, double* work,
                 double* alpha, double* Kinv, double* terms, double* grad, int* info);

/* ---- composite calls: a whole model behind the handle ------------------------------------------------------
 * For callers that are not Python: the sequencing the Python host side (device.py, gpr.py) otherwise provides,
 * as thin C++ over the building blocks above.  HOST pointers in and out; the device buffers (X, normalised
 * targets, factor, leaf inverses, inverse factor, alpha, fp32 serving copies, staging) are owned by the handle, one
 * model per handle (a new gpk_fit / gpk_import replaces it; gpk_model_release or gpk_destroy frees it).
 *
 * gpk_fit: X host (N x D), Y host (N x P) row-major fp64.  ls: n_ls = 1 (isotropic) or D (ARD) length-scales;
 *   K = sf2 exp(-d^2/2) + (noise + jitter) I (`noise`: the WhiteKernel level, `jitter`: the regressor's alpha).
 *   normalize_y != 0: targets are centred and divided by their population std per column (a zero std counts as 1).
 *   Runs K1 -> K2 -> K3 (+ the inverse factor when Np <= 32768) and evaluates the log-marginal likelihood.
 *   Returns GPK_NOT_PD as gpk_potrf does (the caller decides: sklearn raises, the package GP multiplies its noise by
 *   10, gaussian_process.py:193-201).  D <= GPK_MAX_D_PREDICT, P <= GPK_MAX_P.
 *   Replaces: GaussianProcessRegressor.fit at fixed theta, sklearn/gaussian_process/_gpr.py:271-282,343-364, as
 *   called at src/px4/simple_gp.py:170-177; GaussianProcess.fit, gaussian_process.py:173-201.
 * gpk_predict: Xq host (M x D), mean host (M x P), var host (M x P: per-output VARIANCE, already multiplied by
 *   y_std^2; NULL = means only), all of `dtype` (GPK_F64: double buffers, fp64 kernels; GPK_F32: float buffers, the
 *   fp32 serving kernels - matrix-core mean when admissible, fp16 x 2 split variance - behind the two fp32 serving
 *   gates: a model whose fp32 mean would leave 1e-4 (estimated once per model from two fp64 launches on <= 1024 training
 *   rows) is served by the fp64 kernels, and rows whose fp32 variance is below 1 % of the prior's are recomputed by the
 *   fp64 launch; GPK_F32 is a request for speed, the stated bars - mean 1e-4, std 1e-3 - hold either way).
 *   var_includes_noise != 0:
 *   k** = sf2 + noise, variance clipped at 0 (scikit-learn: Sum.diag, _gpr.py:474-485; take sqrt for its std);
 *   == 0: k** = sf2, floored at 1e-10 (gaussian_process.py:229-233).  Queries are processed in panels.
 *   Replaces: GaussianProcessRegressor.predict, _gpr.py:441-494 (src/px4/simple_gp.py:194, mpc.py:1490-1506);
 *   GaussianProcess.predict, gaussian_process.py:203-241.
 * gpk_lml: theta == NULL: *lml = the fitted model's log-marginal likelihood.  Otherwise theta = log [ls (1 or D
 *   values), noise] (n_theta = 2 or D + 1; sf2 and jitter as fitted): *lml and, if grad != NULL, its gradient with
 *   respect to theta (same layout; isotropic: summed over the features), evaluated on scratch buffers - the fitted
 *   factor is not touched.  A non-positive-definite trial matrix gives *lml = -inf, grad = 0 and GPK_OK (what an
 *   optimiser needs, _gpr.py:586-589).  Replaces: log_marginal_likelihood, _gpr.py:537-652 + kernels.py:1571-1580.
 * gpk_export / gpk_import: the model as host arrays - L (N x N row-major lower factor, zeros above the diagonal:
 *   scikit-learn's L_), alpha (N x P), y_mean / y_std (P) - e.g. to write or read the reference's model files
 *   (src/px4/train_gp_offline.py:188-194; gaussian_process.py:369-394 stores the training set and refits).  NULL
 *   outputs are skipped.  An imported model predicts; gpk_lml(theta) needs a fitted one.                        */
GPK_API int gpk_fit(gpk_handle h, const double* X, int64_t N, int D, const double* Y, int P, const double* ls, int n_ls,
            double sf2, double noise, double jitter, int normalize_y);
GPK_API int gpk_predict(gpk_handle h, const void* Xq, int64_t M, void* mean, void* var, int dtype, int var_includes_noise);
GPK_API int gpk_lml(gpk_handle h, const double* theta, int n_theta, double* lml, double* grad);
GPK_API int gpk_export(gpk_handle h, int64_t* N, int* D, int* P, double* L, double* alpha, double* y_mean, double* y_std,
               double* lml);
GPK_API int gpk_import(gpk_handle h, const double* X, int64_t N, int D, const double* L, const double* alpha, int P,
               const double* ls, int n_ls, double sf2, double noise, const double* y_mean, const double* y_std);
GPK_API int gpk_model_release(gpk_handle h);
/* gpk_predict_model_cov: posterior mean and covariance of the model of gpk_fit / gpk_import, fp64 host buffers: Xq (M x D),
 * mean (M x P, un-normalised), cov (P x M x M: output p's block is y_std[p]^2 Sigma, Sigma = K(Xq, Xq) + noise I - V^T V with
 * the model's WhiteKernel level as noise, not clipped).  Up to GPK_HOST_MAX_M queries one call of gpk_predict_host_cov; more
 * (<= 16384) the fused mean and gpk_predict_cov_inv.  Forms the inverse factor if the model does not hold it yet.
 * Replaces: GaussianProcessRegressor.predict(X, return_cov=True), sklearn/gaussian_process/_gpr.py:441-469.             */
GPK_API int gpk_predict_model_cov(gpk_handle h, const double* Xq, int64_t M, double* mean, double* cov);

/* ---- composite calls for B (<= GPK_MAX_BATCH) single-output models on shared inputs ----------------------------
 * The per-axis layout of src/px4/gp_trainer.py:139-179 (one scalar GP per residual component, each with its own ARD
 * length-scales and noise, all on the same X) as one object behind the handle, next to - and independent of - the
 * single model of gpk_fit.  HOST pointers in and out, fp64.
 * gpk_fit_batched: X host (N x D); Y host (N x B), column b = targets of model b; ls host (B x n_ls), n_ls = 1 or D;
 *   sf2, noise: host double[B]; jitter and normalize_y as in gpk_fit, shared.  One Gram launch per model, then ONE
 *   batched launch chain for the B factorisations, inverse factors and alpha solves (gpk_batch_begin).  info: host
 *   int[B], 0 or the 1-based index of model b's first non-positive pivot; if any is non-zero the call returns
 *   GPK_NOT_PD and the batch is not usable for prediction.
 *   Replaces: the loop over outputs of GPTrainer.train_gp_models at fixed theta, gp_trainer.py:139-179 (six times
 *   sklearn/gaussian_process/_gpr.py:271-282,343-364).
 * gpk_predict_batched: Xq host (M x D); mean host (M x B); var host (M x B: variances in target units, NULL = means
 *   only); var_includes_noise as in gpk_predict.  Up to 32 queries (N <= 16384) take gpk_predict_host_multi (one call,
 *   two launches for all models); larger batches one fused mean launch (gpk_predict_mean_multi) and one variance launch
 *   per model and panel.  Replaces: PreTrainedGP.predict_residual's loop, src/px4/pretrained_gp.py:52-98.
 * gpk_lml_batched: thetas == NULL: lml[b] = the fitted models' log-marginal likelihoods.  Otherwise thetas host
 *   (B x n_theta), row b = log [ls (1 or D values), noise] of model b: lml host double[B] and, if grad != NULL, grad
 *   host (B x n_theta), from one batched launch chain on scratch buffers (BASELINE configuration 5: the
 *   hyper-parameter step of all per-axis models at once).  A model whose trial matrix is not positive definite gets
 *   lml = -inf, grad = 0.  Replaces: B evaluations of log_marginal_likelihood, _gpr.py:537-652.
 * gpk_model_release frees this object too.                                                                         */
GPK_API int gpk_fit_batched(gpk_handle h, int B, const double* X, int64_t N, int D, const double* Y, const double* ls, int n_ls,
                    const double* sf2, const double* noise, double jitter, int normalize_y, int* info);
GPK_API int gpk_predict_batched(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var, int var_includes_noise);
GPK_API int gpk_lml_batched(gpk_handle h, const double* thetas, int n_theta, double* lml, double* grad);

/* ---- K9: sparse inducing-point GP - fit on every row, serve through m inducing inputs -----------------------------------
 * The Titsias / DTC ("projected process") predictor of GPflow's SGPR (the reference's src/px4/gp.py is a GPflow model): one
 * kernel sf2 RBF(ls) shared by P outputs, noise sigma^2 = noise (the WhiteKernel level) + jitter (the regressor's alpha),
 * targets normalised with a y_mean / y_std FIXED when the object is created - only then are the statistics additive.  With m
 * inducing inputs Z (mp = gpk_padded(m)) the training rows enter through fp64 statistics of size m x m,
 *     G = Kuf Kfu (m x m),  g = Kuf Yn (m x P),  yy[p] = sum Yn[:, p]^2,  N,
 * kept on the device as ONE symmetric matrix S = F^T F, F = [Kfu | Yn] (rows x (mp + 128)): S[0:mp, 0:mp] = G,
 * S[mp + p][0:mp] = S[0:mp][mp + p] = g[:, p], S[mp + p][mp + p] = yy[p], zero in the padding.  Appending n rows costs n m^2
 * flops and an m x m refactorisation; serving costs what an exact model of m rows costs.  A third object behind the handle,
 * next to the single model and the batch; gpk_model_release and gpk_destroy free it.  HOST pointers and fp64 throughout,
 * except gpk_sparse_accumulate.
 * Replaces: the row caps the reference needs because its exact models cannot train on what a flight log holds -
 *   src/px4/gp_trainer.py:95-96 (a random max_samples), src/px4/train_gp_offline.py:124 (max_data_points = 10000),
 *   quadrotor_gp_mpc/quadrotor_gp_mpc/gaussian_process.py:146-149 and src/px4/simple_gp.py (the oldest rows past 1000 dropped).
 *
 * gpk_sparse_accumulate: the statistics pass, the device-pointer building block: S (dev, nt x ld, nt = mp + 128, even
 *   ld >= nt, 16-byte aligned; symmetric on entry - zero to begin with - and on return) += F^T F over the n rows X (dev n x D),
 *   Yn (dev n x P, normalised targets) against Z (dev m x D); ls host double[D].  Rows go in panels of at most "sparse_panel"
 *   rows (gpk_set_option; 0, the default: F within 128 MiB - half of the Infinity Cache, so that the panel the cross kernel
 *   wrote is still on the chip when the product reads it - between 1024 and 16384 rows).  Per panel: F by exact differences (as
 *   gpk_cross_gram_t), the lower tiles of F^T F on the fp64 matrix cores with the panel's rows cut into k-slabs (independent
 *   products of one launch, one partial matrix each), and one launch that adds the partials IN SLAB ORDER into S and mirrors it
 *   to both halves; a one-slab panel accumulates straight into the lower tiles and one mirror pass ends the call.  No
 *   floating-point atomics: the same sequence of calls gives the same bits; S is symmetric bit for bit.  The slab count is a
 *   function of (mp, panel rows) only - one from 256 lower 128-tiles (the CU count) on, below that the fewest that give 1024
 *   tiles, at most 16, never under 512 rows each - or option "sparse_slabs" (1 .. 64).  Asynchronous; work area: the handle's scratch.  1 <= m <= 16384, D <= 16, P <= GPK_MAX_P.
 * gpk_sparse_begin: creates the object with zero statistics.  Z host (m x D); ls: n_ls = 1 or D values; jitter_uu: absolute,
 *   on the diagonal of Kuu.  1 <= m <= 16384, D <= 16, P <= GPK_MAX_P, noise + jitter > 0.
 * gpk_sparse_update: appends n >= 1 raw rows X (n x D), Y (n x P): checks that they are finite, normalises the targets, runs
 *   the panel loop and synchronises once.
 * gpk_sparse_finalize: assembles the model; any number of updates may precede it, none included (the model is then the
 *   prior), and the statistics stay valid for further updates.
 *       Luu Luu^T = Kuu + jitter_uu I,  Wuu = Luu^-1            (gpk_gram, gpk_potrf, gpk_trtri)
 *       B = I + Wuu G Wuu^T / sigma^2,  LB LB^T = B             (two tile GEMMs; gpk_potrf)
 *       r = Wuu g / sigma^2,  alpha_u = Wuu^T B^-1 r            (tile GEMMs on 128-column panels)
 *       WSigma = LB^-1 Wuu                                      (lower tiles + zeros to their right: the inverse-factor
 *                                                                layout of gpk_predict_var_inv)
 *       bound = sum_p [ -N/2 log(2 pi sigma^2) - sum log diag LB - (N sf2 - sigma^2 (tr B - m)) / (2 sigma^2)
 *                       - yy[p] / (2 sigma^2) + r_p^T B^-1 r_p / 2 ]          (gpk_lml_terms on (LB, r, B^-1 r))
 *   the collapsed lower bound on the log-marginal likelihood in normalised-target units; the exact value when Z = X.
 *   Returns GPK_NOT_PD with *info = the 1-based pivot, as gpk_potrf, if Kuu + jitter_uu I or B is not positive definite.
 * gpk_sparse_predict: the semantics of gpk_predict at GPK_F64: Xq (M x D), mean (M x P, un-normalised),
 *       mean(x) = y_mean + y_std k_u(x)^T alpha_u,   var_f(x) = sf2 - |Wuu k_u(x)|^2 + |WSigma k_u(x)|^2,
 *   var (M x P: variance times y_std^2; NULL = means only); var_includes_noise != 0: + the WhiteKernel level, clipped at 0;
 *   == 0: floored at 1e-10.  Checks that the queries are finite.  Up to 32 queries (D, P <= 16): the two-factor form of the
 *   small-batch kernels - small_cross_mean_kernel with ONE model (one K*, all P outputs), then small_var_kernel with the
 *   inverse factor (0: Wuu, 1: WSigma) as its second grid dimension; the last workgroup overall adds each factor's shares in the
 *   one-factor kernel's order and writes max((kss - t0) - (0 - t1), floor) y_std[p]^2: the mean one launch, mean + variance
 *   two, one synchronisation, for every P, and the bits of the route it replaces (gpk_predict_host_multi with B = 2, for
 *   P > 1 two gpk_predict_host calls, combined on the host).  More queries, or option small_path = 0: panels of the fused
 *   mean and two gpk_predict_var_inv launches.
 * gpk_sparse_predict_grad: the semantics and units of gpk_predict_model_grad on the sparse posterior, host fp64 buffers: Xq
 *   (M x D), mean (M x P), dmean (M x P x D) un-normalised; var (M x P) and dvar (M x P x D) already multiplied by
 *   y_std[p]^2, or both NULL.  With k = k_u(x), u_jd = (z_jd - x_d) / ls_d^2:
 *       dmean[m][p][d] = y_std[p] sum_j k_mj u_jd alpha_u[j][p]
 *       dvar[m][d]     = -2 sum_j k_mj u_jd (c0 - c1)_jm,   c0 = Wuu^T (Wuu k),  c1 = WSigma^T (WSigma k)
 *   dvar is the gradient of the UNCLIPPED variance; var is clipped as gpk_sparse_predict clips it.  Any M >= 1.  Up to 32
 *   queries: the two-factor small-batch kernels - mean + Jacobian ONE launch (small_cross_mean_jac_kernel), all four results
 *   three (+ small_var_grad_kernel, small_wtv_grad_kernel: the factor is blockIdx.y / z, both read the same K*, each keeps
 *   its own V and shares, one ticket count over both, dvar = -2 / ls_d (s0 - s1) by the last workgroup), one synchronisation,
 *   queries and results through the pinned, mapped block.  More, or option small_path = 0: query panels of gpk_predict_mean,
 *   gpk_predict_mean_grad and gpk_predict_var_grad_inv once per inverse factor (floor -DBL_MAX; kss = 0 for WSigma), combined
 *   by one small launch; one synchronisation per panel.
 *   Replaces: nothing in the reference (GPflow's SGPR behind src/px4/gp.py would differentiate predict_f by reverse mode; the
 *   consumer is the linearisation of quadrotor_gp_mpc/quadrotor_gp_mpc/mpc_controller.py:318); within this library, what
 *   gpk_predict_model_grad is to the exact model, without forming two "models" (two K*, two mean shares).
 * gpk_sparse_predict_cov: the semantics of gpk_predict_model_cov on the sparse posterior: mean (M x P, un-normalised), cov
 *   (P x M x M: output p's block is y_std[p]^2 Sigma),
 *       Sigma = K(Xq, Xq) + noise I - V0^T V0 + V1^T V1,   V0 = Wuu K*^T,  V1 = WSigma K*^T,
 *   the model's WhiteKernel level on the diagonal only, not clipped, symmetric bit for bit.  1 <= M <= 16384.  Up to 32
 *   queries: two launches (small_cross_mean_kernel, small_cov_kernel: the factor is blockIdx.y, group sums per factor, one top
 *   ticket over the groups of both; (k(a, b) - s0) + s1, mirrored), one synchronisation.  More, or option small_path = 0: the
 *   stacked panel [V0; V1] by two tile GEMMs, its copy [V0; -V1], and ONE symmetric tile GEMM of depth 2 mp with the
 *   covariance epilogue (gpk_predict_cov_inv's).
 *   Replaces: GPflow's predict_f(full_cov=True) of the SGPR model behind src/px4/gp.py; the consumer is the sampling of
 *   sklearn/gaussian_process/_gpr.py:497-537 (sample_y).
 *   Both entries check that a finalised model exists and that the queries are finite, and refuse batched mode.
 * gpk_sparse_bound: the bound of the last gpk_sparse_finalize and the rows seen so far.
 * gpk_sparse_export / gpk_sparse_import: Z (m x D), the statistics G (m x m), g (m x P), yy (P), n_rows and the
 *   hyper-parameters - ls (n_ls values), hyper = [sf2, noise, jitter, jitter_uu], y_mean, y_std (P) - as host arrays; NULL
 *   outputs are skipped.  The importer then only finalises (and may go on updating).
 *
 * FITC (Snelson & Ghahramani 2006): the other standard inducing-point posterior.  DTC treats the part of a training row that
 * the inducing inputs cannot explain, k_ii - k_i^T Kuu^-1 k_i, as zero; FITC gives the row that residual as noise of its own.
 * It differs from DTC in the statistics only.  With Wuu = Luu^-1 and
 *       q_i = |Wuu k_u(x_i)|^2,   lambda_i = sigma^2 + max(sf2 - q_i, 0),   w_i = sigma^2 / lambda_i  in (0, 1]
 * the statistics are S = F^T diag(w) F - G = Kuf diag(w) Kfu, g = Kuf diag(w) Yn, yy[p] = sum w_i Yn[i][p]^2 - and the assembly
 * of gpk_sparse_finalize, unchanged, yields the FITC posterior: mean k_u^T alpha_u, variance sf2 - |Wuu k_u|^2 + |WSigma k_u|^2,
 * Q = Kuu^-1 - Sigma~.  Every entry that serves a finalised object (gpk_sparse_predict*, the _multi entries, paths, propagate,
 * moments) therefore serves a FITC object as it is.  The statistics stay additive over rows at fixed (Z, hyper-parameters);
 * the likelihood needs one more additive scalar, sum_i log lambda_i.
 * Replaces: GPflow's GPRFITC, which the reference's GPflow variant (src/px4/gp.py) could have used; nothing in the reference
 *   serves it.
 * gpk_sparse_accumulate_fitc: the weighted statistics pass, the device-pointer building block beside gpk_sparse_accumulate: its
 *   operands, then Wuu (dev, mp x ldw, even ldw >= mp, 16-byte aligned: the inverse factor of Kuu + jitter_uu I in the layout
 *   gpk_trtri writes), sigma2 = noise + jitter > 0, log_lambda_sum (dev double[1]: sum_i log lambda_i is ADDED to what it
 *   holds) and w (dev, n doubles, or NULL: receives the weights).  S += F^T diag(w) F.  The panel rule, the k-slab rule, the
 *   limits and the work area (the handle's scratch) of gpk_sparse_accumulate; the panel is written in whole 128-row blocks.
 *   Per panel, between the panel kernel and the F^T F launches, which run unchanged on the scaled panel:
 *     the q_i without storing V = Kfu Wuu^T - ONE tile GEMM Wuu F[:, 0:mp]^T (the k-tiles in the zero triangle of Wuu skipped)
 *       whose sum-of-squares epilogue leaves one partial per (tile row of Wuu, row of the panel): gpk_predict_var_inv's launch
 *       with the panel in the place of a second kernel matrix.  Option "fitc_fused" = 0: gpk_predict_var_inv itself on the
 *       panel's rows (a second kernel-matrix pass and its own finalising launch) - the composed route, kept as the check;
 *     one launch that adds the partials in tile order, forms lambda_i and w_i, multiplies row i of F (all mp + 128 columns, the
 *       targets included) by sqrt(w_i) in place and writes one sum of log lambda_i per 64-row workgroup (rows >= n of the last
 *       block stay zero and contribute nothing);
 *     one launch that adds those sums in a fixed order onto log_lambda_sum.
 *   No floating-point atomics, flags or spins: the same sequence of calls gives the same bits, S stays symmetric bit for bit.
 *   Asynchronous.
 * gpk_sparse_set_approximation: kind = GPK_SPARSE_DTC (0, what gpk_sparse_begin / gpk_sparse_import create) or GPK_SPARSE_FITC
 *   (1).  Legal while the object has seen no rows (none updated, held or imported); afterwards GPK_BAD_ARG with a message,
 *   unless kind repeats the current one (then nothing happens).  Choosing FITC factors Kuu + jitter_uu I and forms Wuu at once -
 *   the pass needs them before the first row; GPK_NOT_PD with *info = the pivot as in gpk_sparse_finalize, which factors again
 *   (the same launches: the finalised bits do not depend on it).  On a FITC object gpk_sparse_update and gpk_sparse_hold run
 *   the weighted pass; gpk_sparse_eval[_z] set the hyper-parameters (and Z), factor Kuu FIRST, accumulate the held rows again
 *   with the weights and return the value - with grad != NULL or gradZ != NULL they return GPK_BAD_ARG with a message that
 *   names FITC before anything is launched or changed: where lambda depends on the hyper-parameters and on Z the gradient is a
 *   different one, and it is not built.  gpk_sparse_finalize and gpk_sparse_bound return, on a FITC object, the FITC
 *   log-marginal likelihood log N(y | 0, Qff + diag(lambda)) in normalised-target units,
 *       sum_p [ -N/2 log(2 pi) - 1/2 sum_i log lambda_i - sum log diag LB - yy[p] / (2 sigma^2) + r_p^T B^-1 r_p / 2 ]
 *   - the DTC formula with -N/2 log sigma^2 replaced and no trace term; it equals the DTC bound, and the exact value, when
 *   Z = X.  gpk_sparse_select is unaffected.
 * gpk_sparse_get_approximation: kind and sum_i log lambda_i over the rows seen (0 for DTC; synchronises); NULL outputs are skipped.
 * gpk_sparse_restore_approximation: beside gpk_sparse_import - sets kind and the sum as gpk_sparse_get_approximation returned
 *   them for the imported statistics (FITC: factors Kuu as the setter does); the object can then finalise and go on taking
 *   rows.  GPK_BAD_ARG on an object that holds rows.
 *
 * Training: the gradient of the bound L with respect to log [ls .., noise, sf2] (jitter and jitter_uu do not depend on them).
 * Replaces: the optimiser loop of GPflow's SGPR behind the reference's src/px4/gp.py (gpflow.optimizers.Scipy().minimize on
 *   model.training_loss, which differentiates the same collapsed bound by reverse mode over the N x m cross-covariance), and
 *   the exact-model fits on capped rows that stand in for it (src/px4/gp_trainer.py:163-180, GaussianProcessRegressor with
 *   n_restarts_optimizer on max_samples rows).
 * With Kuu^-1, Sigma~ = (Kuu + G / s2)^-1, alpha_u = Sigma~ g / s2 the partial derivatives are
 *       dL/dg = alpha_u / s2,   dL/dG = P / (2 s2) (Kuu^-1 - Sigma~) - alpha_u alpha_u^T / (2 s2),
 *       dL/dKuu = P / 2 (Kuu^-1 - Sigma~) - P / (2 s2) Kuu^-1 G Kuu^-1 - alpha_u alpha_u^T / 2
 *   and with F = [Kfu | Yn], C = [2 dL/dG ; dL/dg^T] ((m + P) x m), Q = F C (N x m)
 *       dL/dlog ls_d = sum_ni Q_ni Kfu_ni ((x_nd - z_id) / ls_d)^2 + sum_ij dL/dKuu_ij Kuu0_ij ((z_id - z_jd) / ls_d)^2
 *       dL/dlog sf2  = sum Q o Kfu + sum dL/dKuu o Kuu0 - P N sf2 / (2 s2)        (Kuu0 = Kuu without jitter_uu)
 *       dL/dlog noise = noise [ P (-N / (2 s2) + N sf2 / (2 s2^2) - tr(Kuu^-1 G) / (2 s2^2) + tr(Sigma~ G) / (2 s2^2))
 *                               + sum yy / (2 s2^2) - sum alpha_u o g / s2^2 + tr(alpha_u^T G alpha_u) / (2 s2^2) ].
 * gpk_sparse_grad_pass: the sums over the rows, the device-pointer building block beside gpk_sparse_accumulate: sums (dev
 *   double[17]) [d] = sum_ni Q_ni Kfu_ni ((x_nd - z_id) / ls_d)^2 for d < D, [16] = sum_ni Q_ni Kfu_ni, Q = [Kfu | Yn] Cm; Cm dev
 *   (mp + 128) x ldc (even ldc >= mp, 16-byte aligned): rows [0, m) and [mp, mp + P), columns [0, m), ZERO elsewhere.  Per
 *   panel of rows (the panel rule of gpk_sparse_accumulate): F again, ONE tile GEMM on the fp64 matrix cores (rows x mp, k =
 *   mp + 128) whose epilogue never stores Q - each tile multiplies its accumulators by the matching entries of F and by the
 *   squared scaled differences recomputed from X and Z, and writes 17 sums - and a fixed-order reduction of the tiles' sums into
 *   the running sums.  No floating-point atomics: the same calls give the same bits.  Asynchronous; work area: the handle's
 *   scratch.  The limits of gpk_sparse_accumulate.
 * gpk_sparse_hold: n raw rows X (n x D), Y (n x P), host: checked to be finite, normalised with the object's y_mean / y_std and
 *   kept on the device; the statistics are REPLACED by those of these rows.  n == 0 releases the held rows (the statistics
 *   stay); so does a later gpk_sparse_update (they would no longer be the statistics' rows).
 * gpk_sparse_eval: sets the hyper-parameters (ls: n_ls values, n_ls as at gpk_sparse_begin; jitter, jitter_uu, y_mean, y_std
 *   stay), accumulates the statistics of the held rows again, assembles the model as gpk_sparse_finalize does (same return
 *   codes: GPK_NOT_PD with *info = the pivot) and returns the bound; grad != NULL: also its gradient, grad[n_ls + 2] =
 *   d/dlog [ls .., noise, sf2] (n_ls == 1: the features' sum).  The gradient forms Kuu^-1, Sigma~ (gpk_wtw), Kuu^-1 G Kuu^-1 and
 *   G alpha_u (tile GEMMs) in buffers of the assembly that the served model does not need, runs the row pass and takes the Kuu
 *   term from gpk_lml_grad's pass on (Z, alpha_u, Kuu^-1 - Sigma~ - Kuu^-1 G Kuu^-1 / s2): one synchronisation more than the
 *   assembly.  After a successful call the object is the finalised model at these hyper-parameters.
 *   GPK_BAD_ARG without held rows.
 *
 * Training the inducing inputs: the gradient of the bound with respect to Z.
 * Replaces: GPflow's SGPR behind the reference's src/px4/gp.py keeps inducing_variable.Z a trainable parameter, and the same
 *   gpflow.optimizers.Scipy().minimize differentiates the collapsed bound with respect to it together with the kernel - that is
 *   how a small m summarises many rows.
 * With T = Q o Kfu (Q = F C as above), GammaK = dL/dKuu = (P / 2) M - alpha_u alpha_u^T / 2, M = Kuu^-1 - Sigma~ - Kuu^-1 G Kuu^-1 / s2:
 *       dL/dz_id = (U_id + V_id) / ls_d,
 *       U_id = sum_n T_ni (x_nd / ls_d - z_id / ls_d),          V_id = 2 sum_j GammaK_ij Kuu0_ij (z_jd / ls_d - z_id / ls_d)
 *   by differences of the length-scale-divided coordinates (never T^T X - z sum T: two large sums that cancel).  y_mean / y_std,
 *   jitter and jitter_uu do not depend on Z; an isotropic kernel uses the same formula with equal ls_d.
 * gpk_sparse_zgrad_pass: the column pass, the device-pointer building block beside gpk_sparse_grad_pass (same operands, same
 *   limits, same panel loop and scratch, asynchronous): R (dev, gpk_padded(m) x 17) [i][d] = U_id for d < D (zero for D <= d <
 *   16), [i][16] = sum_n T_ni; rows i >= m are zero.  Per panel of rows: F again, ONE tile GEMM whose epilogue never stores Q -
 *   each tile multiplies its accumulators by the matching entries of F and by the scaled differences, sums them over its rows
 *   (lane, lane groups, waves: a fixed order) and writes 17 sums per column - and a launch that adds the row-tiles' sums in
 *   tile order into R, panel after panel.  No floating-point atomics: the same calls give the same bits.
 * gpk_sparse_eval_z: gpk_sparse_eval with the inducing inputs as arguments.  Z != NULL (host m x D; m and D are the object's;
 *   checked to be finite) replaces the object's inducing inputs, Z == NULL keeps them; then gpk_sparse_eval: the statistics of
 *   the held rows are accumulated again (against the new Z), the model is assembled (same return codes: GPK_NOT_PD with *info =
 *   the pivot), bound and grad as there.  gradZ != NULL (host m x D): dL/dZ in raw coordinates - behind the launches of the
 *   hyper-parameter gradient the matrix M is mirrored to a full matrix, one m x m kernel forms V (one inducing input per
 *   workgroup, j in index order, Kuu0 recomputed by exact differences) and the column pass U; still one synchronisation.
 *   After a successful call the object is the finalised model at these hyper-parameters and this Z, and gpk_sparse_export
 *   returns it.  With Z == NULL and gradZ == NULL the launches and the bits are gpk_sparse_eval's.
 *
 * Choosing the inducing inputs: greedy conditional-variance selection (Burt, Rasmussen, van der Wilk, JMLR 2020), a pivoted
 * partial Cholesky factorisation of Kff = K(X, X) that never forms Kff.
 * Replaces: the random caps the reference puts on its rows - src/px4/gp_trainer.py:95-96 (np.random.choice of max_samples
 *   rows) and the deque caps quoted above - as the way to pick which rows stand for the log.
 * With d_i = sf2 for every row, step t = 0, 1, .. takes j = the LOWEST index among the rows with the largest d and stops, with
 * *selected = t, if t == m_max, or d_j <= min_var sf2, or (t >= 1 and sum_i d_i <= tol n sf2); otherwise dmax[t] = d_j,
 * idx[t] = j and
 *       c_i  = sf2 exp(-1/2 sum_d ((x_id - x_jd) / ls_d)^2) - sum_{s < t} l_is l_js        (s ascending)
 *       l_it = c_i / sqrt(d_j),   d_i = max(d_i - l_it^2, 0),   d_j = 0 exactly,
 *       trace[t] = sum_i d_i      ( = tr(Kff - Kfu Kuu^-1 Kuf) with Z = X[idx[0 .. t]]: the trace term of the collapsed bound).
 * The kernel value is formed as gpk_cross_gram_t forms it; every sum runs in an order fixed by (n, m_max); no floating-point
 * atomics: the same call gives the same bits.  Entries of idx / trace / dmax from *selected on are not written.
 * gpk_greedy_select_bytes: the size of gpk_greedy_select's work area in bytes - the transposed panel (m_max x ldn doubles, ldn
 *   = n rounded up to 32), the scaled coordinates (16 x ldn), d (ldn) and the workgroups' partials; 0 for sizes that
 *   gpk_greedy_select refuses.
 * gpk_greedy_select: the device-pointer building block.  X dev (n x D); ls host, n_ls = 1 or D values; work dev, 16-byte
 *   aligned, gpk_greedy_select_bytes(n, m_max) bytes, supplied by the caller (262 144 rows x 4096 columns are 8.6 GB: not a
 *   temporary of the handle); idx dev int64[m_max], trace and dmax dev double[m_max], selected dev int64[1].  One launch
 *   per pivot between an initialising and a closing launch, m_max + 2 in all, on the handle's stream: every workgroup of step t
 *   reduces the per-workgroup (largest d, lowest index, sum of d) that step t - 1 left, in the same order, so that all reach
 *   the same pivot and the same stop decision - after a stop the remaining launches return at once; no host round trip, no
 *   ticket, flag or spin: the launch boundary is the only hand-off.  Asynchronous.  1 <= m_max <= min(n, 16384), D <= 16.
 * gpk_sparse_select: the host entry, with the kernel hyper-parameters of the sparse object behind the handle.  X host (n x D,
 *   checked to be finite), or NULL: the rows that gpk_sparse_hold keeps on the device (n must be their count; GPK_BAD_ARG
 *   without held rows).  idx (int64), trace, dmax: host arrays of m_max entries, of which the first *selected are written.
 *   Allocates and frees its own work area (GPK_HIP_ERROR if the device cannot hold it), synchronises once and leaves the
 *   object's model, statistics and inducing inputs untouched.  Refuses batched mode.                                     */
GPK_API size_t gpk_greedy_select_bytes(int64_t n, int64_t m_max);
GPK_API int gpk_greedy_select(gpk_handle h, const double* X, int64_t n, int D, const double* ls, int n_ls, double sf2,
                              int64_t m_max, double min_var, double tol, void* work, int64_t* idx, double* trace, double* dmax,
                              int64_t* selected);
GPK_API int gpk_sparse_select(gpk_handle h, const double* X, int64_t n, int64_t m_max, double min_var, double tol, int64_t* idx,
                              double* trace, double* dmax, int64_t* selected);
GPK_API int gpk_sparse_accumulate(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m, int D,
                                  int P, const double* ls, double sf2, double* S, int64_t ld);
GPK_API int gpk_sparse_grad_pass(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m, int D,
                                 int P, const double* ls, double sf2, const double* Cm, int64_t ldc, double* sums);
GPK_API int gpk_sparse_zgrad_pass(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m, int D,
                                  int P, const double* ls, double sf2, const double* Cm, int64_t ldc, double* R);
GPK_API int gpk_sparse_begin(gpk_handle h, const double* Z, int64_t m, int D, int P, const double* ls, int n_ls, double sf2,
                             double noise, double jitter, double jitter_uu, const double* y_mean, const double* y_std);
GPK_API int gpk_sparse_hold(gpk_handle h, const double* X, const double* Y, int64_t n);
GPK_API int gpk_sparse_eval(gpk_handle h, const double* ls, int n_ls, double sf2, double noise, double* bound, double* grad,
                            int* info);
GPK_API int gpk_sparse_eval_z(gpk_handle h, const double* Z, const double* ls, int n_ls, double sf2, double noise, double* bound,
                              double* grad, double* gradZ, int* info);
GPK_API int gpk_sparse_update(gpk_handle h, const double* X, const double* Y, int64_t n);
GPK_API int gpk_sparse_finalize(gpk_handle h, int* info);
GPK_API int gpk_sparse_predict(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var, int var_includes_noise);
GPK_API int gpk_sparse_predict_grad(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var, double* dmean,
                                    double* dvar, int var_includes_noise);
GPK_API int gpk_sparse_predict_cov(gpk_handle h, const double* Xq, int64_t M, double* mean, double* cov);

/* ---- K9, the per-axis batch: B single-output sparse models served on one query batch ----------------------------------------
 * The model file a controller loads holds six scalar GPs, each with its own ARD length-scales and noise level; the exact models
 * have gpk_predict_host_multi[_grad|_cov] for that shape.  These are the same for sparse objects: 1 <= B <= 8 handles, behind
 * each a FINALISED sparse object with P = 1, all with the same m and D and on the same device - each with its own inducing
 * inputs, alpha_u, length-scales, sf2, noise, target normalisation and factor pair (Wuu, WSigma).  h is the serving handle
 * (it may be one of `models`): it supplies the stream, the pinned staging block, the work area and the ticket counters.
 * Host fp64 buffers in the per-axis layout: Xq (M x D), mean and var (M x B), dmean and dvar (M x B x D), cov (B x M x M).
 * Units, clipping and flooring PER MODEL exactly as gpk_sparse_predict / _grad / _cov: mean un-normalised; var, dvar and cov
 * block b already times y_std_b^2; var_includes_noise != 0 adds model b's WhiteKernel level and clips at 0, == 0 floors at
 * 1e-10; dvar is the gradient of the unclipped variance; cov block b has noise_b on its diagonal and is symmetric bit for bit.
 * var == NULL: means only (multi_grad: var and dvar come together or not at all).
 *
 * Up to 32 queries (option small_path on): the two-factor small-batch kernels with a model dimension - the first launch
 * (small_cross_mean[_jac]_kernel) takes the model as blockIdx.y: one K* and one set of mean / Jacobian shares per model; the
 * variance, covariance and W^T V launches take 2 * model + factor as the grid dimension that is the factor in the single
 * entries: per (model, factor) its own rows of V, shares, group sums and group counters, per model ONE ticket count over the
 * workgroups of both of its factors, and that model's last workgroup writes max((kss - t0) - (0 - t1), floor) y_std^2,
 * (k(a, b) - s0) + s1 mirrored, dvar = -2 / ls_d (s0 - s1).  For every B: means one launch, mean + variance two, mean +
 * Jacobian one, all four gradient results three, mean + covariance two; one synchronisation per call.  No flags, spins or
 * floating-point atomics; every sum runs in an order fixed by (mp, M) alone, so model b's block of every result has the bits
 * of gpk_sparse_predict[_grad|_cov] on that model alone (B = 1 IS that route).  All ticket counters are left at zero.
 * More queries, or option small_path = 0: model by model through the panel routes of the single entries on h's stream (one
 * synchronisation per panel and model) - the cross-check of the kernels above.
 *
 * The entries read the models' device buffers across handles.  Those are stable once gpk_sparse_finalize, gpk_sparse_eval[_z]
 * or gpk_sparse_import + gpk_sparse_finalize on that object have returned (they synchronise, through gpk_lml_terms), and stay
 * so until the next call that changes that object; the entry synchronises nothing on the models' own streams, and no such
 * call may run on a model while the entry does.
 * GPK_BAD_ARG with a message, before anything is launched or read: B outside [1, 8], a NULL handle, an object that is missing,
 * not finalised, on another device, with P != 1 or with another m or D, M < 1 (cov: M > 16384), non-finite queries, var
 * without dvar, batched mode.
 * Replaces: six gpk_sparse_predict* calls - six synchronisations - per control step for the six residual models of
 *   src/px4/pretrained_gp.py:52-98 (predict_residual) once they are sparse; nothing in the reference serves a
 *   sparse model.                                                                                                          */
GPK_API int gpk_sparse_predict_multi(gpk_handle h, int B, const gpk_handle* models, const double* Xq, int64_t M, double* mean,
                                     double* var, int var_includes_noise);
GPK_API int gpk_sparse_predict_multi_grad(gpk_handle h, int B, const gpk_handle* models, const double* Xq, int64_t M, double* mean,
                                          double* var, double* dmean, double* dvar, int var_includes_noise);
GPK_API int gpk_sparse_predict_multi_cov(gpk_handle h, int B, const gpk_handle* models, const double* Xq, int64_t M, double* mean,
                                         double* cov);
/* The input Hessian of the sparse posterior mean (K8, second derivatives).  The sparse mean is that of an exact model over
 * (Z, alpha_u) and its Hessian involves no inverse factor, so these are gpk_predict_model_hess on the inducing inputs:
 * gpk_sparse_predict_hess: host fp64 buffers Xq (M x D), mean (M x P), dmean (M x P x D), hess (M x P x D x D); mean and dmean
 *   have the bits of gpk_sparse_predict_grad.  Up to 32 queries: the two launches of gpk_predict_host_hess on (Z, alpha_u),
 *   one synchronisation; larger batches in query panels of the general blocks.  Any M.
 * gpk_sparse_predict_multi_hess: B (<= 8) single-output sparse models as gpk_sparse_predict_multi_grad takes them, each with
 *   its own inducing inputs; mean (M x B), dmean (M x B x D), hess (M x B x D x D); column b has the bits of models[b] alone.
 *   Up to 32 queries: the same two launches for all models (the model grid dimension, per-model basis points); larger
 *   batches model by model.
 * A null hess is GPK_BAD_ARG.  Replaces: nothing in the reference; within this library 2 D gpk_sparse_predict_grad calls.  */
GPK_API int gpk_sparse_predict_hess(gpk_handle h, const double* Xq, int64_t M, double* mean, double* dmean, double* hess);
GPK_API int gpk_sparse_predict_multi_hess(gpk_handle h, int B, const gpk_handle* models, const double* Xq, int64_t M, double* mean,
                                          double* dmean, double* hess);
GPK_API int gpk_sparse_bound(gpk_handle h, double* bound, int64_t* n_rows);
GPK_API int gpk_sparse_export(gpk_handle h, int64_t* m, int* D, int* P, int* n_ls, double* Z, double* G, double* g, double* yy,
                              int64_t* n_rows, double* ls, double* hyper, double* y_mean, double* y_std);
GPK_API int gpk_sparse_import(gpk_handle h, const double* Z, int64_t m, int D, int P, const double* ls, int n_ls, double sf2,
                              double noise, double jitter, double jitter_uu, const double* y_mean, const double* y_std,
                              const double* G, const double* g, const double* yy, int64_t n_rows);
#define GPK_SPARSE_DTC 0
#define GPK_SPARSE_FITC 1
GPK_API int gpk_sparse_accumulate_fitc(gpk_handle h, const double* X, const double* Yn, int64_t n, const double* Z, int64_t m, int D,
                                       int P, const double* ls, double sf2, double* S, int64_t ld, const double* Wuu, int64_t ldw,
                                       double sigma2, double* log_lambda_sum, double* w);
GPK_API int gpk_sparse_set_approximation(gpk_handle h, int kind, int* info);
GPK_API int gpk_sparse_get_approximation(gpk_handle h, int* kind, double* log_lambda_sum);
GPK_API int gpk_sparse_restore_approximation(gpk_handle h, int kind, double log_lambda_sum, int* info);

/* ---- building block: whole-tile GEMM on the matrix cores ---------------------------------------
 * C[m x n] = alpha * opA(A) * opB(B)^T + beta * C, m and n multiples of 128, k a multiple of 16
 * (fp64) / 32 (fp32).  ta == 0: A stored (m x k) with k contiguous; ta == 1: A stored (k x m).
 * tb == 0: B stored (n x k); tb == 1: B stored (k x n).  lower_only != 0 skips tiles strictly above
 * the diagonal.  This is the kernel behind gpk_potrf / gpk_potrs / gpk_trsm_lower_left / gpk_potri;
 * it is exported so that it can be tested and timed on its own (fp64 via v_mfma_f64_16x16x4_f64,
 * fp32 via v_mfma_f32_32x32x2_f32).  No reference counterpart other than the BLAS-3 calls inside
 * LAPACK's dpotrf/dtrsm (SciPy, sklearn/gaussian_process/_gpr.py:349,454).                          */
GPK_API int gpk_gemm_tiles(gpk_handle h, int dtype, int ta, int tb, const void* A, int64_t lda, const void* B,
                   int64_t ldb, void* C, int64_t ldc, int64_t m, int64_t n, int64_t k, double alpha,
                   double beta, int lower_only);

/* ---- K10: posterior function draws (pathwise conditioning) ----------------------------------------------------------
 * A posterior draw of the exact model as an explicit function (Wilson et al. 2020, "Efficiently sampling functions from
 * Gaussian process posteriors"), in normalised-target units:
 *     f_s(x) = phi(x)^T w_s + k(x, X) v_s,   v_s = K^-1 (y_n - Phi w_s - eps_s),   K = k(X, X) + (noise + alpha) I,
 *     phi_f(x) = sqrt(2 sf2 / F) cos(omega_f . x + phase_f),  omega_f ~ N(0, diag(1 / ls^2)),  phase_f ~ U(0, 2 pi),
 *     w_s ~ N(0, I_F),  eps_s ~ N(0, (noise + alpha) I);  the only approximation is the finite F of the prior term.
 * A path set for S paths and P outputs is ONE coefficient matrix Coef: (N + F) rows x C = S P columns, row-major, column
 * s P + p, leading dimension ldc >= C, NO row padding: rows [0, N) hold v (the weights on k(x, x_j)), rows [N, N + F) hold
 * sqrt(2 sf2 / F) w (the weights on cos(omega_f . x + phase_f)).  With it go Omega (dev, F x D), phase (dev, F) and the
 * model's X (dev, N x D), ls (host, D), sf2, y_mean / y_std (host, P).  The value served is y_mean[p] + y_std[p] f_s(x).
 * Limits of the family: 1 <= D <= GPK_MAX_D_PREDICT, 1 <= P <= GPK_MAX_P, 1 <= S <= 4096, 1 <= F <= 16384, N >= 1,
 * 1 <= H <= 256 (GPK_BAD_ARG otherwise); fp64; not available in batched mode.  No reference counterpart (the reference
 * evaluates marginal moments only, sklearn/gaussian_process/_gpr.py:367-496); scikit-learn's sample_y (:498-535) draws at a
 * fixed batch and cannot follow a rollout whose next query depends on the last draw.
 *
 * gpk_rff_features: Phi[n][f] = scale cos(omega_f . x_n + phase_f) for n < N, f < F, zero elsewhere in the
 *   (gpk_padded(N) x gpk_padded(F)) block that gpk_gemm_tiles takes; Phi dev, ldp >= gpk_padded(F).  Elementwise,
 *   asynchronous.  Exported so that it can be tested alone.
 * gpk_paths_prepare: the set-up (not the hot path).  W_rand (dev, F x C) = the w_s, Eps (dev, N x C) = the eps_s, column
 *   s P + p both; Yn (dev, N x P) the normalised targets; W (dev, Np x ldw) the inverse factor L^-1 of K (gpk_trtri),
 *   Np = gpk_padded(N).  R = Yn (x) 1_S - Phi W_rand - Eps, V = W^T (W R) - the tile GEMM, three launches - and Coef is
 *   written as laid out above.  Work area: the handle's scratch ((Np Fp + Fp Cp + 2 Np Cp) doubles).  Asynchronous.
 *   gpk_padded(N) + gpk_padded(F) <= 65535.
 * gpk_paths_step: the hot path.  Xq (dev, S x D): path s is evaluated at ITS OWN row s,
 *     out[s][p] = y_mean[p] + y_std[p] sum_{j < N + F} b_j(xq_s) Coef[j][s P + p]
 *     b_j(x) = sf2 exp(-0.5 ||(x - x_j) / ls||^2) for j < N (exact differences),  cos(omega_{j-N} . x + phase_{j-N}) above;
 *   out dev (S x P).  Two launches: a grid of (64-path blocks) x (row chunks) in which every coefficient row is read once, as
 *   contiguous runs, and the basis value is formed once per (s, j); then the chunks' shares added in chunk order.  No
 *   floating-point atomics; the chunk count depends on (N + F, S) only: the same bits every call.  Bound by streaming Coef,
 *   (N + F) S P 8 bytes.  Work area: the handle's scratch.  Asynchronous.
 * gpk_paths_rollout: a horizon in one call.  Host inputs x0 (x0_rows x P, x0_rows = S or 1: one start for every path),
 *   U (H x (D - P); NULL if D == P), lin (P x D); the state dimension is P <= D.  Stage h, every path s:
 *     q_s = [x_s, U[h]],   x_s <- x_s + lin q_s + out_s(q_s)
 *   with the advance fused into the second launch of gpk_paths_step, so that the next stage's queries never leave the
 *   device.  traj (host, (H + 1) x S x P) receives the trajectory, stage 0 = x0.  2 H launches, one synchronisation.
 *   x0, U and lin must be finite (GPK_BAD_ARG: "NaN or infinity").                                                       */
GPK_API int gpk_rff_features(gpk_handle h, const double* X, int64_t N, int D, const double* Omega, const double* phase,
                             int64_t F, double scale, double* Phi, int64_t ldp);
GPK_API int gpk_paths_prepare(gpk_handle h, const double* X, int64_t N, int D, const double* Yn, int P, const double* W,
                              int64_t Np, int64_t ldw, const double* Omega, const double* phase, int64_t F, double sf2,
                              const double* W_rand, const double* Eps, int S, double* Coef, int64_t ldc);
GPK_API int gpk_paths_step(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2, const double* Omega,
                           const double* phase, int64_t F, const double* Coef, int64_t ldc, int S, int P, const double* y_mean,
                           const double* y_std, const double* Xq, double* out);
GPK_API int gpk_paths_rollout(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2, const double* Omega,
                              const double* phase, int64_t F, const double* Coef, int64_t ldc, int S, int P, const double* y_mean,
                              const double* y_std, const double* x0, int x0_rows, const double* U, int H, const double* lin,
                              double* traj);

/* ---- K10, the per-axis batch: B single-output models on shared inputs X, each with its own kernel ---------------------
 * A batch path set for B models (1 <= B <= 8), S paths and F features is ONE coefficient matrix Coef: (N + F) rows x ldc
 * columns, row-major, MODEL-MAJOR columns: model b, path s is column b mstride + s, mstride >= S, ldc >= B mstride (columns
 * in the padding are never read or written).  Rows [0, N) hold v_b, rows [N, N + F) hold sqrt(2 sf2_b / F) w_b.  With it go
 * Omega (dev, B x F x D), phase (dev, B x F), the shared X (dev, N x D) and per model ls (host, B x D), sf2 (host, B) and an
 * output pair shift / scale (host, B): the value served is shift[b] + scale[b] f_{b,s}(x).  The set-up is B calls of
 * gpk_paths_prepare with P = 1 on Coef + b mstride with the batch's ldc, each with that model's inverse factor, Omega_b,
 * phase_b and sf2_b: no new device code, and model b's column block has the bits of its own single-model path set.
 * Limits: those of the family above with 1 <= B <= 8 in the place of P; GPK_BAD_ARG with a message before any launch.
 *
 * gpk_paths_step_multi: the hot path.  Xq (dev, S x D): path s of EVERY model is evaluated at row s,
 *     out[s][b] = shift[b] + scale[b] sum_{j < N + F} b_{j,b}(xq_s) Coef[j][b mstride + s]
 *     b_{j,b}(x) = sf2_b exp(-0.5 ||(x - x_j) / ls_b||^2) for j < N,  cos(omega_{b,j-N} . x + phase_{b,j-N}) above;
 *   out dev (S x B).  Two launches: a grid of (64-path blocks) x (row chunks) in which lane l owns path 64 block + l for the
 *   basis values and the products alike, the difference x - x_j is formed once per (s, j) for all models and every
 *   coefficient is read once, as B contiguous runs of 64 doubles per wave and row; then the chunks' shares added in chunk
 *   order.  No floating-point atomics; the chunking is gpk_paths_step's, a function of (N + F, S) only, and so are the
 *   summation order and the expression forms: column b of out has the BITS of gpk_paths_step on model b's own path set
 *   (P = 1, y_mean = shift[b], y_std = scale[b]) at the same queries.  Work area: the handle's scratch.  Asynchronous.
 * gpk_paths_rollout_multi: a horizon in one call, in RAW units.  Host inputs: nx (the state dimension, B <= nx <= D),
 *   coord (B, distinct, in [0, nx)): the state coordinate model b's output is added to; in_shift / in_scale (D; both NULL:
 *   identity): the input scaler the models were fitted behind; x0 (x0_rows x nx, x0_rows = S or 1), U (H x (D - nx); NULL
 *   if D == nx), lin (nx x D).  Stage h, every path s:
 *     q_s = [x_s, U[h]],   z_s = (q_s - in_shift) / in_scale,   x_s <- x_s + lin q_s + sum_b e_coord[b] out_b(z_s)
 *   a coordinate without a model advances by lin alone.  The advance is fused into the second launch, which writes the
 *   next stage of the trajectory where the next stage's first launch reads its queries.  traj (host, (H + 1) x S x nx),
 *   stage 0 = x0.  2 H launches, one synchronisation.  x0, U, lin and the scaler must be finite, in_scale non-zero.     */
GPK_API int gpk_paths_step_multi(gpk_handle h, const double* X, int64_t N, int D, int B, const double* ls, const double* sf2,
                                 const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                                 int64_t mstride, int S, const double* shift, const double* scale, const double* Xq,
                                 double* out);
GPK_API int gpk_paths_rollout_multi(gpk_handle h, const double* X, int64_t N, int D, int B, const double* ls, const double* sf2,
                                    const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                                    int64_t mstride, int S, const double* shift, const double* scale, int nx, const int* coord,
                                    const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                    const double* U, int H, const double* lin, double* traj);

/* ---- K10, the sparse models: paths conditioned on the inducing variables ------------------------------------------------
 * Pathwise conditioning on u = f(Z) (Wilson et al. 2020, the sparse case), in normalised-target units, on the assembled model
 * of the handle (gpk_sparse_finalize: Wuu = Luu^-1, WS = LB^-1 Wuu, alpha_u; Wuu^T Wuu = (Kuu + jitter_uu I)^-1):
 *     f_s(x) = phi(x)^T w_s + k_u(x)^T v_s,   v_s = alpha_u + WS^T xi_s - Wuu^T (Wuu Phi_Z w_s),   xi_s ~ N(0, I_m),  w_s ~ N(0, I_F)
 * phi, omega and phase as above.  With xi = 0 and w = 0 the value is gpk_sparse_predict's mean; the ensemble covariance is
 * A A^T + B B^T with B = k_u WS^T - exactly the + |WS k*|^2 term of the sparse variance - and A = phi^T - k_u Kuu^-1 Phi_Z,
 * which tends to K** - |Wuu k*|^2 as F grows.  A sparse path set is therefore the coefficient matrix of the family above with
 * N := m and X := Z: rows [0, m) hold v, rows [m, m + F) hold sqrt(2 sf2 / F) w, and gpk_paths_step / gpk_paths_rollout serve
 * it unchanged.  Every output of a multi-output model draws its own xi and w: column s P + p, alpha_u's column p.
 *
 * gpk_sparse_paths_prepare: the set-up (not the hot path).  Omega (dev, F x D), phase (dev, F), W_rand (dev, F x C) = the w_s,
 *   Xi (dev, m x C) = the xi_s, C = S P, column s P + p both.  Coef (dev, (m + F) x ldc, ldc >= C, no row padding) receives
 *   the matrix; columns [C, ldc) are not written.  Zdst (dev, m x D) receives a copy of the model's inducing inputs: the path
 *   set owns everything it needs and stays the same function after the model is refitted or freed.  Launches:
 *   gpk_rff_features on Z, a pack kernel (zero-padded W_rand and Xi), four tile GEMMs with the triangular k-ranges of
 *   gpk_potrs_inv - T = Phi_Z Wr, T <- Wuu T, R = -Wuu^T T, R += WS^T Xi - and an unpack that adds alpha_u's column p and
 *   writes the scaled w rows.  Padding: rows [m, mp) of Phi_Z and of the packed Xi are zeros, and Wuu and WS are both the
 *   IDENTITY on the padding's diagonal with zeros between padding and model (Kuu + jitter_uu I is the identity there, so are
 *   Luu and Luu^-1; B is, so is LB^-1, and WS = LB^-1 Wuu is the product of the two: the identity, not the zeros of the
 *   memset it is written over) - so every product's padding rows are exact zeros, nothing of them reaches a row below m,
 *   and the unpack reads no row at or above m.  Work area: the handle's scratch ((mp Fp + Fp Cp + 3 mp Cp) doubles).
 *   Asynchronous.  GPK_BAD_ARG with a message before any launch: no assembled model (as gpk_sparse_predict), batched mode,
 *   gpk_padded(m) + gpk_padded(F) > 65535, S not in [1, 4096], F not in [1, 16384], ldc < C, a null pointer.
 * gpk_paths_step_multi_z / gpk_paths_rollout_multi_z: gpk_paths_step_multi / gpk_paths_rollout_multi, argument for argument,
 *   with Zs (dev, B x N x D: model b's basis points at Zs + b N D) in the place of the shared X: the batch of B sparse
 *   models, each with its own inducing inputs (N = m).  For j < N model b reads its own x_j and the difference is formed per
 *   model; expression forms, row, wave and chunk order, the chunking (a function of (N + F, S)) and the second launch are
 *   those of the shared form, so column b of the result has the BITS of gpk_paths_step on model b's own path set
 *   (X = Zs_b, P = 1, y_mean = shift[b], y_std = scale[b]).  The same limits and refusals.                               */
GPK_API int gpk_sparse_paths_prepare(gpk_handle h, const double* Omega, const double* phase, int64_t F, const double* W_rand,
                                     const double* Xi, int S, double* Coef, int64_t ldc, double* Zdst);
GPK_API int gpk_paths_step_multi_z(gpk_handle h, const double* Zs, int64_t N, int D, int B, const double* ls, const double* sf2,
                                   const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                                   int64_t mstride, int S, const double* shift, const double* scale, const double* Xq,
                                   double* out);
GPK_API int gpk_paths_rollout_multi_z(gpk_handle h, const double* Zs, int64_t N, int D, int B, const double* ls, const double* sf2,
                                      const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                                      int64_t mstride, int S, const double* shift, const double* scale, int nx, const int* coord,
                                      const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                      const double* U, int H, const double* lin, double* traj);

/* ---- K10, path gradients: the input Jacobian of every path beside its value ----------------------------------------------
 * A path is a closed form, f_s(x) = sum_{j<N} v_js k(x, x_j) + sum_{f<F} c_fs cos(omega_f . x + phase_f), and so is its gradient:
 *     d b_j / d x_d = -b_j(x) (x_d - x_jd) / ls_d^2   (j < N),     d b_{N+f} / d x_d = -sin(omega_f . x + phase_f) omega_fd
 * Each entry below is the entry it is named after, argument for argument, plus jac; limits and refusals are the family's,
 * a null jac is GPK_BAD_ARG with a message, and every refusal happens before any launch.  The served Jacobian carries the
 * output scale (y_std[p]; scale[b]); y_mean and shift do not enter.
 * Two launches per stage, as the value entries.  The first has the outputs (up to three p of a model, which share the basis value;
 * one b of a batch) in the grid's third dimension: lane l owns
 * path 64 block + l for the basis value, the product and the D derivative sums - RBF rows add e t_d with e = b_j c_j and the
 * t_d = (x_d - x_jd) / ls_d the value forms, cosine rows add sin(t) c omega_d - over the chunking of gpk_paths_step, rows,
 * waves and chunks in its order; the second adds the shares in chunk order, RBF and cosine shares apart, and writes
 * jac = scale * -(sum_rbf / ls_d + sum_cos).  No floating-point atomics: the same bits every call.
 *   VALUE BITS: out (traj) has the bits of the value entry on the same arguments - the value is formed by the value kernels'
 *   expressions in their order.
 *   BATCH BITS: column b of a batch jac has the bits of gpk_paths_step_grad's jac on model b's own path set (P = 1, y_mean =
 *   shift[b], y_std = scale[b], X = Zs_b for _z) - both layouts run the same kernels.
 * Work area: the handle's scratch (per stage (chunks + (chunks + 1) D) columns doubles; a rollout's jac H times over).
 *
 * gpk_paths_step_grad: jac (dev, S x P x D), jac[s][p][d] = d out[s][p] / d Xq[s][d].
 * gpk_paths_step_multi_grad / _z: jac (dev, S x B x D), jac[s][b][d] = d out[s][b] / d Xq[s][d] (the query as given: scaled).
 * gpk_paths_rollout_grad: jac (host, H x S x P x D): jac[h][s][p][d] is the derivative of stage h's residual out_s (evaluated
 *   at traj[h]) w.r.t. coordinate d of q_s = [x_s, U[h]].  One more copy back, the same one synchronisation.
 * gpk_paths_rollout_multi_grad / _z: jac (host, H x S x B x D), as above for out_b, in the RAW units of q: it includes the
 *   input scaler's 1 / in_scale[d].                                                                                       */
GPK_API int gpk_paths_step_grad(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2, const double* Omega,
                                const double* phase, int64_t F, const double* Coef, int64_t ldc, int S, int P,
                                const double* y_mean, const double* y_std, const double* Xq, double* out, double* jac);
GPK_API int gpk_paths_rollout_grad(gpk_handle h, const double* X, int64_t N, int D, const double* ls, double sf2,
                                   const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc, int S,
                                   int P, const double* y_mean, const double* y_std, const double* x0, int x0_rows,
                                   const double* U, int H, const double* lin, double* traj, double* jac);
GPK_API int gpk_paths_step_multi_grad(gpk_handle h, const double* X, int64_t N, int D, int B, const double* ls, const double* sf2,
                                      const double* Omega, const double* phase, int64_t F, const double* Coef, int64_t ldc,
                                      int64_t mstride, int S, const double* shift, const double* scale, const double* Xq,
                                      double* out, double* jac);
GPK_API int gpk_paths_rollout_multi_grad(gpk_handle h, const double* X, int64_t N, int D, int B, const double* ls,
                                         const double* sf2, const double* Omega, const double* phase, int64_t F, const double* Coef,
                                         int64_t ldc, int64_t mstride, int S, const double* shift, const double* scale, int nx,
                                         const int* coord, const double* in_shift, const double* in_scale, const double* x0,
                                         int x0_rows, const double* U, int H, const double* lin, double* traj, double* jac);
GPK_API int gpk_paths_step_multi_grad_z(gpk_handle h, const double* Zs, int64_t N, int D, int B, const double* ls,
                                        const double* sf2, const double* Omega, const double* phase, int64_t F, const double* Coef,
                                        int64_t ldc, int64_t mstride, int S, const double* shift, const double* scale,
                                        const double* Xq, double* out, double* jac);
GPK_API int gpk_paths_rollout_multi_grad_z(gpk_handle h, const double* Zs, int64_t N, int D, int B, const double* ls,
                                           const double* sf2, const double* Omega, const double* phase, int64_t F,
                                           const double* Coef, int64_t ldc, int64_t mstride, int S, const double* shift,
                                           const double* scale, int nx, const int* coord, const double* in_shift,
                                           const double* in_scale, const double* x0, int x0_rows, const double* U, int H,
                                           const double* lin, double* traj, double* jac);

/* ---- K11: horizon propagation - the posterior's mean rollout with the linearised state covariance, one call -------------
 * The first-order propagation of Hewing, Kabzan and Zeilinger (Cautious MPC using GP regression): state x in R^nx, query
 * q = [x, u] in R^D, lin (nx x D) the nominal increment as in gpk_paths_rollout[_multi].  For rollout r and stage h:
 *   z = (q - in_shift) / in_scale;  mu_b, J_b = d mu_b / d q (RAW units: includes 1 / in_scale[d]) and v_b the posterior mean,
 *   its Jacobian and the variance of output b at z, in target units: v_b = y_std[b]^2 (max(kss - |W k*|^2, floor) [+ noise]);
 *   x_{h+1}     = x_h + lin q + sum_b e_coord[b] mu_b
 *   A_h         = I + lin[:, :nx] + sum_b e_coord[b] J_b[:nx]
 *   Sigma_{h+1} = A_h Sigma_h A_h^T + sum_b v_b e_coord[b] e_coord[b]^T + Q
 * A coordinate without a model advances by lin alone and receives no variance.  fp64 only.  Host arrays in, host arrays out:
 *   x0 (x0_rows x nx, rows = R or 1), U (u_rows x H x nu, rows = R or 1, nu = D - nx; NULL if nu = 0), lin (nx x D),
 *   Sigma0 (s_rows x nx x nx, rows = R or 1; NULL: zero; the LOWER triangle is read and mirrored), Q (nx x nx or NULL: zero;
 *   the lower triangle is read);  traj ((H + 1) x R x nx), Sigma ((H + 1) x R x nx x nx, every block symmetric bit for bit),
 *   and optionally (NULL: not wanted) the stage quantities exactly as used: mean and var (H x R x P or B), jac (H x R x P or
 *   B x D).  var_includes_noise != 0 adds `noise` (normalised-target units, per model in the batch form) to the clipped variance.
 * Launches: per stage the two small-batch launches "mean + Jacobian + variance" (gpk_small.hip; mean, var and jac of a stage
 * have the BITS of gpk_predict_host_grad / gpk_predict_host_multi_grad called on the R rows [traj[h], U[h]], scaled) and one
 * advance launch (one workgroup per rollout, sequential fixed-order sums): 3 H launches, one copy in before the chain, up to five
 * out after it, ONE stream synchronisation at the end and none between the stages (the caller's arrays are pageable host memory:
 * the runtime stages the copies to and from them and may wait on them by itself).  Repeatable bit for bit.  Work area: the
 * handle's scratch.
 * gpk_propagate_host: one exact model with P outputs; the state is its outputs (nx = P <= D), no input scaler.  Model
 *   arguments as gpk_predict_host_grad.
 * gpk_propagate_host_multi: B <= 8 single-output models, model arguments as gpk_predict_host_multi_grad; nx, coord (B distinct
 *   state coordinates), in_shift / in_scale (D each, both or neither) as gpk_paths_rollout_multi.  RAW units.
 * GPK_BAD_ARG (with a message, before any launch): R not in [1, 32], H not in [1, 256], nx or D above 16, nx > D, nx < B,
 *   gpk_padded(N) > 16384, Np != gpk_padded(N), ldw < Np, a wrong row count ("x0 / U / Sigma0 must have 1 or R rows"), NaN or
 *   infinity in a host input ("x0, U, lin and Q must not contain NaN or infinity", "Sigma0 must not contain NaN or infinity";
 *   the model's ls, sf2, y_mean, y_std, kss, floor and noise included), a length-scale that is not positive, in_scale zero,
 *   coord out of range or repeated, a null pointer, batched mode.  The checks of R, H, the row counts, the horizon's null
 *   pointers and its finiteness are the same code, with these messages, for every propagation entry of this header
 *   (gpk_propagate*, gpk_sparse_propagate*, gpk_propagate_mm_host*).                                                          */
GPK_API int gpk_propagate_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                               double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np, int64_t ldw,
                               double kss, double floor_, int var_includes_noise, double noise, const double* x0, int x0_rows,
                               const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q,
                               int R, int H, double* traj, double* Sigma, double* mean, double* var, double* jac);
GPK_API int gpk_propagate_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                     const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                     const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                     int var_includes_noise, const double* noise, int nx, const int* coord,
                                     const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                     const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                     const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                     double* jac);

/* ... on the sparse posteriors: the same chain - the recursion, the host arrays, 3 H launches, one upload, up to five downloads,
 * ONE stream synchronisation - on the two-factor small-batch launches (kss - |Wuu k*|^2 + |WSigma k*|^2 on m inducing
 * points), m in the place of N: R in [1, 32], H in [1, 256], nx <= D <= 16, gpk_padded(m) <= 16384.
 * gpk_sparse_propagate: the finalised sparse object of h, P outputs; the state is its outputs (nx = P <= D), no scalers.
 *   Replaces: H calls of gpk_sparse_predict_grad - H synchronisations and H W^T V launches whose result the recursion never
 *   reads - around the composition on the host; in the reference, nothing (its GP-MPC propagates no covariance).
 * gpk_sparse_propagate_multi: B <= 8 handles of finalised single-output models of equal m and D, handle rules as
 *   gpk_sparse_predict_multi_grad (h supplies the stream and the scratch; nothing is synchronised on the models' own
 *   streams); nx, coord, in_shift / in_scale as gpk_propagate_host_multi; out_shift / out_scale (B each, both or neither): the
 *   affine map out_shift[b] + out_scale[b] y behind every model's output, folded into the y_mean / y_std the kernels apply.
 *   RAW units.  Replaces: H calls of gpk_sparse_predict_multi_grad around the composition on the host.
 * Stage quantities (mean, var: H x R x P or B; jac: H x R x P or B x D) in the units of gpk_sparse_predict[_multi]_grad.  With
 * var_includes_noise != 0 mean, jac and var have the BITS of that entry (its last argument 1) at the rows [traj[h], U[h]].  With
 * 0 var is the latent variance of gpk_sparse_predict_grad(..., 0): kss = sf2, clipped at 1e-10 (normalised-target units) -
 * where a host loop over the noisy entry forms max(noisy - noise y_std^2, 0); the two differ in rounding only while neither
 * clip is active.
 * GPK_BAD_ARG (with a message, before any launch): no finalised sparse model (in the batch: any handle), models that disagree
 *   in m or D or have several outputs, B outside 1..8, the limits above, nx < B, a wrong row count, NaN or infinity in a host
 *   input, in_scale zero, coord out of range or repeated, a scaler given by half, a null pointer, batched mode, option
 *   small_path = 0.  Timed under GPK_TIMED_PROPAGATE as the exact entries.                                                  */
GPK_API int gpk_sparse_propagate(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U, int u_rows,
                                 const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H, double* traj,
                                 double* Sigma, double* mean, double* var, double* jac);
GPK_API int gpk_sparse_propagate_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                       const int* coord, const double* in_shift, const double* in_scale, const double* out_shift,
                                       const double* out_scale, const double* x0, int x0_rows, const double* U, int u_rows,
                                       const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H,
                                       double* traj, double* Sigma, double* mean, double* var, double* jac);

/* ... at second order in the mean: for x ~ N(xbar, Sigma), E[mu(x)] = mu(xbar) + tr(H Sigma) / 2 + O(Sigma^2), H the mean's
 * input Hessian; the term is of the order of the covariance the chain carries.  The four entries above with two more arguments:
 * order (1 or 2, anything else GPK_BAD_ARG with a message) and corr (H x R x P or B, may be NULL).  With order = 2
 *   c_b         = 1/2 sum_{d,e < nx} H_b[d][e] Sigma_h[d][e]      H_b = d^2 mu_b / d q^2 in RAW units at q = [x_h, u_h]
 *   x_{h+1}     = (x_h + lin q + sum_b e_coord[b] mu_b) + sum_b e_coord[b] c_b      (c added LAST, as one addition)
 *   A_h, Sigma_{h+1}: as at first order, at the same query
 * The controls are exact, so only the nx x nx block of H enters; A_h stays the Jacobian at x_h (the derivative of c holds third
 * derivatives).  No Hessian is formed: with delta_j = (z - X_j) / ls and St[d][e] = Sigma_h[d][e] / (in_scale_d ls_d in_scale_e
 * ls_e) (model b's own length-scales),
 *   tr(H_b Sigma_h) = y_std[b] sum_j k*_j alpha_jb (delta_j^T St delta_j - tr St)
 * R x P (or B) scalars per stage.  Launches: 4 H - per stage the two small-batch launches, unchanged; one trace launch (at most
 * 64 workgroups per model, each its rows' share of the two sums, K* recomputed from the device queries, Sigma_h read from the
 * chain's state; no ticket, no atomics); the advance launch, which adds the shares in workgroup order.  One upload, ONE
 * synchronisation, one more download when corr is given.  traj and Sigma of stage h + 1 and mean, var, jac of stage h are the
 * first-order quantities at the (corrected) query of stage h: with H = 1 Sigma[1], mean, var and jac have the BITS of order 1
 * and traj[1] = traj_order1[1] + corr[0] (scattered to coord) exactly.  corr[h] is c of stage h.  With order = 1 the entries
 * return the bits of their first-order siblings and corr is zero-filled.  The sparse pair takes (Z, alpha_u) as the mean's
 * model, as gpk_sparse_predict_hess; its batch form folds out_scale into y_std, which scales c as it scales the mean.
 * Limits, refusals and timing (GPK_TIMED_PROPAGATE brackets the advance launch) as above.                                   */
GPK_API int gpk_propagate2_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np, int64_t ldw,
                                double kss, double floor_, int var_includes_noise, double noise, const double* x0, int x0_rows,
                                const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q,
                                int R, int H, double* traj, double* Sigma, double* mean, double* var, double* jac, int order,
                                double* corr);
GPK_API int gpk_propagate2_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                      const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                      const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                      int var_includes_noise, const double* noise, int nx, const int* coord,
                                      const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                      const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                      const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                      double* jac, int order, double* corr);
GPK_API int gpk_sparse_propagate2(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U, int u_rows,
                                  const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H, double* traj,
                                  double* Sigma, double* mean, double* var, double* jac, int order, double* corr);
GPK_API int gpk_sparse_propagate2_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                        const int* coord, const double* in_shift, const double* in_scale, const double* out_shift,
                                        const double* out_scale, const double* x0, int x0_rows, const double* U, int u_rows,
                                        const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H,
                                        double* traj, double* Sigma, double* mean, double* var, double* jac, int order,
                                        double* corr);

/* ... with the gradient of a horizon cost l(X, Sigma) with respect to the controls, the start state and the start covariance
 * (order 1 only): the four first-order entries with five more arguments.  The caller supplies the seeds
 *   gx (H + 1 x R x nx) = dl/dx_h,   gS (H + 1 x R x nx x nx) = dl/dSigma_h, entries taken as independent (NULL: zero); the
 *   entry uses (gS + gS^T) / 2
 * and receives dU (R x H x nu; NULL when nu = 0), dx0 (R x nx) and dSigma0 (R x nx x nx, may be NULL) - one row per rollout,
 * also where x0, U or Sigma0 came as one shared row.  The forward recursion is the one above; the backward sweep starts from
 * lam_H = gx_H, Lam_H = sym(gS_H) and runs, for h = H - 1 .. 0 and c_b = coord[b],
 *   F_h   = [I 0] + lin + sum_b e_c J_b                      (nx x D: all D columns of the Jacobian, RAW units)
 *   G_h   = Lam_{h+1} A_h Sigma_h
 *   w_b   = [G_h[c_b, :nx], 0 .. 0]
 *   g_q   = F_h^T lam_{h+1} + sum_b Lam_{h+1}[c_b][c_b] grad_q v_b + 2 sum_b H_b w_b        (H_b = d^2 mu_b / d q^2, RAW units)
 *   lam_h = gx_h + g_q[:nx],   dU_h = g_q[nx:],   Lam_h = sym(gS_h) + A_h^T Lam_{h+1} A_h   (lower triangle formed and mirrored)
 * dx0 = lam_0, dSigma0 = Lam_0 (symmetric bit for bit).  grad v_b is the gradient of the unclipped variance, as
 * gpk_predict_host[_multi]_grad / gpk_sparse_predict[_multi]_grad return it; it does not depend on var_includes_noise.  No
 * Hessian is formed: with delta_j = (z - X_j) / ls, k_j = sf2 exp(-|delta_j|^2 / 2) and wh_d = w_d / (ls_d in_scale_d) (model b's
 * own length-scales)
 *   (H_b w)_e = y_std[b] / (ls_e in_scale_e) (sum_j alpha_jb k_j delta_je (delta_j . wh) - wh_e sum_j alpha_jb k_j)
 * - D + 1 sums per (rollout, output).  Launches: 6 H.  Forward, per stage: the three small-batch launches of the gradient
 * entries (mean, Jacobian, variance and its gradient; mean, Jacobian and variance with the bits of the two-launch stage) and
 * the unchanged advance launch; the scaled queries, Sigma_h, the Jacobians and the variance gradients of every stage stay on
 * the device, H R (D + nx^2 + outputs 2 D) doubles.  Backward, per stage: one Hessian-vector launch (at most 64 workgroups
 * per model, each its rows' share of the sums, K* recomputed from the stored queries, its own rows of G_h formed from the
 * device state; no ticket, no atomics, no inverse factor) and one adjoint launch (one workgroup per rollout; it adds the
 * shares in workgroup order).  One upload with the seeds included, ONE synchronisation, the downloads after it.  traj, Sigma,
 * mean, var and jac have the BITS of the first-order sibling on the same arguments.  The sparse pair takes (Z, alpha_u) as the
 * mean's model, as gpk_sparse_predict_hess.
 *   Replaces: the reverse sweep on the host around H calls of gpk_predict_host[_multi]_grad and H calls of
 *   gpk_predict_host[_multi]_hess (the sparse pair: gpk_sparse_predict[_multi]_grad / _hess) - 2 H synchronisations and
 *   H R outputs D^2 Hessian entries through host memory, of which the sweep reads one contraction per output - or
 *   2 H nu + 1 calls of the first-order sibling for central differences; in the reference, nothing.
 * Limits and refusals are the siblings'; also GPK_BAD_ARG (with a message, before any launch, the outputs untouched): NULL gx
 * or dx0, NULL dU with nu > 0, NaN or infinity in a seed.                                                                  */
GPK_API int gpk_propagate_grad_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                    double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np,
                                    int64_t ldw, double kss, double floor_, int var_includes_noise, double noise, const double* x0,
                                    int x0_rows, const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                    const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                    double* jac, const double* gx, const double* gS, double* dU, double* dx0, double* dSigma0);
GPK_API int gpk_propagate_grad_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                          const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                          const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                          int var_includes_noise, const double* noise, int nx, const int* coord,
                                          const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                          const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                          const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                          double* jac, const double* gx, const double* gS, double* dU, double* dx0,
                                          double* dSigma0);
GPK_API int gpk_sparse_propagate_grad(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U,
                                      int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H,
                                      double* traj, double* Sigma, double* mean, double* var, double* jac, const double* gx,
                                      const double* gS, double* dU, double* dx0, double* dSigma0);
GPK_API int gpk_sparse_propagate_grad_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                            const int* coord, const double* in_shift, const double* in_scale,
                                            const double* out_shift, const double* out_scale, const double* x0, int x0_rows,
                                            const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                            const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                            double* jac, const double* gx, const double* gS, double* dU, double* dx0,
                                            double* dSigma0);

/* ---- K11, exact moment matching: the posterior at GAUSSIAN queries, and the horizon built on it -------------------------
 * For [C.]RBF[+White] models the posterior's moments at a query q ~ N(m, Sigma) have a closed form (Girard; Quinonero-Candela;
 * Deisenroth).  Sigma is non-zero in the leading nx x nx (state) block of the query alone; with z = (q - in_shift) / in_scale,
 * S = Sigma / (in_scale in_scale^T), nu_i = x_i - E[z], Lam_b = diag(ls_b^2), P_b = Lam_b^-1:
 *   l_i          = sf2_b |I + S P_b|^(-1/2) exp(-nu_i^T (S + Lam_b)^-1 nu_i / 2)
 *   E[mu_b]      = sum_i alpha_i l_i,       Cov[z, mu_b] = S (S + Lam_b)^-1 sum_i alpha_i l_i nu_i
 *   L^ab_ij      = |R|^(-1/2) k_a(x_i, m) k_b(x_j, m) exp((P_a nu_i + P_b nu_j)^T R^-1 S (P_a nu_i + P_b nu_j) / 2),  R = S (P_a + P_b) + I
 *   E[mu_a mu_b] = sum_ij alpha_i^a alpha_j^b L^ab_ij,      E[v_b] = kss_b - sum_ij (K_b^-1)_ij L^bb_ij
 *   V_ab         = E[mu_a mu_b] - E[mu_a] E[mu_b] + [a == b] (max(E[v_b], floor) [+ noise])
 * (one exponential per pair of rows, its exponent summed first; L is never stored).  Kinv: dev Np x ldk, the LOWER triangle of the
 * inverse of the model's Gram matrix with its noise / jitter, as gpk_wtw writes it from the inverse factor; its identity padding
 * is masked.  Results in RAW units: mean = y_mean + y_std E[mu], cov = y_std y_std^T V (symmetric bit for bit), xcov[o][d] =
 * Cov[q_d, y_o] = in_scale[d] y_std[o] Cov[z_d, mu_o] (zero for d >= nx).  fp64 only.
 * gpk_moments_host: one model with P outputs (all output pairs share one L).  M <= 32 host queries Xq (M x D) with covariances
 *   Sq (M x nx x nx, the lower triangle is read; NULL: zero) -> mean (M x P), cov (M x P x P), xcov (M x P x D).
 * gpk_moments_host_multi: B <= 8 single-output models, each on its own inputs, model arguments as gpk_predict_host_multi;
 *   B (B + 1) / 2 pairs -> mean (M x B), cov (M x B x B), xcov (M x B x D).  in_shift / in_scale (D each, both or neither).
 * Launches (gpk_moments.hip): the set-up (one wave per query and model or pair: the nx <= 16 factorisations), the row pass (two
 *   launches: l_i with the shares of E[mu] and Cov; w_i and lam_i per pair and side), the pair pass (64 x 64 tiles of the N x N
 *   pairs, for a == b the lower tiles with the others counted twice; every K^-1 and alpha tile read once for all M queries; sums
 *   added in a fixed order, no atomics) and the finishing launch: five launches, one upload, three downloads, ONE synchronisation.
 *   Repeatable bit for bit; query m has the bits of the same query served alone.  Work area: the handle's scratch.
 * GPK_BAD_ARG (with a message, before any launch, the outputs untouched): M not in [1, 32], nx or D above 16, nx > D,
 *   gpk_padded(N) > 16384, Np != gpk_padded(N), ldk < Np, a NULL Kinv or any other null pointer, NaN or infinity in a query, a
 *   covariance or the model's host arrays, a length-scale or sf2 that is not positive, in_scale zero, batched mode.
 *   The covariances must be positive semi-definite (the Python layer refuses others): the entries do not test it, and an
 *   indefinite one gives the set-up's factorisations a pivot that is not positive, hence NaN or infinity in the results.
 *   Replaces: nothing in the reference (its GP-MPC queries deterministic inputs); in the literature an O(N^2 P^2) pass on the CPU. */
GPK_API int gpk_moments_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                             double sf2, const double* y_mean, const double* y_std, const double* Kinv, int64_t Np, int64_t ldk,
                             double kss, double floor_, int var_includes_noise, double noise, int nx, const double* Xq,
                             const double* Sq, int M, double* mean, double* cov, double* xcov);
GPK_API int gpk_moments_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                   const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                   const double* const* Kinv, int64_t Np, int64_t ldk, const double* kss, double floor_,
                                   int var_includes_noise, const double* noise, int nx, const double* in_shift,
                                   const double* in_scale, const double* Xq, const double* Sq, int M, double* mean, double* cov,
                                   double* xcov);
/* The horizon of gpk_propagate_host[_multi] with every stage's moments exact instead of linearised: with A0 = I + lin[:, :nx], E
 * the selector of coord and Cx the state rows of the stage's xcov,
 *   x_{h+1}     = x_h + lin q + E mean
 *   Sigma_{h+1} = A0 Sigma_h A0^T + A0 Cx E^T + E Cx^T A0^T + E cov E^T + Q        (to first order Cx = Sigma_h J_x^T: the sibling's)
 * The arguments of the siblings with Kinv (as above; per model in the batch form) and ldk in the place of W and ldw, and the
 * optional stage outputs (NULL: not wanted) mean (H x R x P or B), cov (H x R x P x P or B x B), xcov (H x R x P or B x D) exactly
 * as used: they have the BITS of gpk_moments_host[_multi] at the R Gaussian queries ([traj[h], U[h]], Sigma[h]).  Per stage the
 * five launches above, the last of which also composes the stage (GPK_TIMED_PROPAGATE brackets it) and writes the next stage's
 * queries on the device: 5 H launches, one upload, up to five downloads, ONE synchronisation.  Sigma is symmetric bit for bit;
 * rollout r of a batch has the bits of that rollout alone.
 * GPK_BAD_ARG (with a message, before any launch, the outputs untouched): the siblings' refusals (W and ldw apart), a Sigma0 with
 * a non-finite entry, a NULL Kinv, ldk < Np.                                                                                   */
GPK_API int gpk_propagate_mm_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                  double sf2, const double* y_mean, const double* y_std, const double* Kinv, int64_t Np,
                                  int64_t ldk, double kss, double floor_, int var_includes_noise, double noise, const double* x0,
                                  int x0_rows, const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                  const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* cov,
                                  double* xcov);
GPK_API int gpk_propagate_mm_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                        const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                        const double* const* Kinv, int64_t Np, int64_t ldk, const double* kss, double floor_,
                                        int var_includes_noise, const double* noise, int nx, const int* coord,
                                        const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                        const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                        const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* cov,
                                        double* xcov);
/* The adjoint of the moments: gpk_moments_host[_multi] with, for l = <gmean, mean> + <(gcov + gcov^T) / 2, cov> + <gxcov, xcov>, the
 * gradients dXq (M x D) = dl/dXq and dSq (M x nx x nx, symmetric bit for bit) = dl/dSq in raw units.  The seeds gmean (M x NO), gcov
 * (M x NO x NO) and gxcov (M x NO x D; columns >= nx, where xcov is zero, are ignored) are host arrays, NULL: zero.  mean, cov and
 * xcov have the BITS of gpk_moments_host[_multi].  The clip passes the seed where E[v] > floor and nothing where it is active; the
 * noise level is a constant.  Closed form (gpk_moments.hip, "the adjoint"): per pair of rows the forward's one exponential, one
 * scalar weight c_ij and the sums of c_ij L_ij {1, zeta_ij, zeta_ij zeta_ij^T} - 1 + D + nx (nx + 1) / 2 sums whatever P is; S is
 * never inverted, so Sq = 0 and a rank-deficient Sq stay legal.  Launches: the forward's five, one that keeps E[mu] and the clip
 * indicators, and four of the adjoint (set-up, row pass, pair pass on the forward's tiles and query groups, finishing launch): ten
 * launches, one upload, five downloads, ONE synchronisation; no atomics; repeatable bit for bit; query m has the bits of the
 * same query served alone.
 * GPK_BAD_ARG (with a message, before any launch, the outputs untouched): the siblings' refusals, a seed with NaN or infinity, a
 * NULL dXq or dSq.                                                                                                              */
GPK_API int gpk_moments_vjp_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                 double sf2, const double* y_mean, const double* y_std, const double* Kinv, int64_t Np, int64_t ldk,
                                 double kss, double floor_, int var_includes_noise, double noise, int nx, const double* Xq,
                                 const double* Sq, int M, double* mean, double* cov, double* xcov, const double* gmean,
                                 const double* gcov, const double* gxcov, double* dXq, double* dSq);
GPK_API int gpk_moments_vjp_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                       const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                       const double* const* Kinv, int64_t Np, int64_t ldk, const double* kss, double floor_,
                                       int var_includes_noise, const double* noise, int nx, const double* in_shift,
                                       const double* in_scale, const double* Xq, const double* Sq, int M, double* mean, double* cov,
                                       double* xcov, const double* gmean, const double* gcov, const double* gxcov, double* dXq,
                                       double* dSq);
/* gpk_propagate_mm_host[_multi] with the gradient of a horizon cost l(traj, Sigma): the siblings' arguments followed by the seeds
 * gx (H + 1, R, nx) = dl/dx_h and gS (H + 1, R, nx, nx) = dl/dSigma_h (NULL: zero; (gS + gS^T) / 2 is used) and the results dU (R,
 * H, nu; NULL only when nu = 0), dx0 (R, nx), dSigma0 (R, nx, nx; may be NULL), as gpk_propagate_grad_host[_multi].  From lam_H =
 * gx_H, Lam_H = sym gS_H, for h = H - 1 .. 0 the stage's moments are seeded with E^T lam (mean), E^T Lam E (cov) and 2 E^T Lam A0
 * (the state columns of xcov), and with (m~, S~) their adjoint at ([x_h, u_h], Sigma_h):
 *   g_q = [I 0]^T lam + lin^T lam + m~,   lam_h = gx_h + g_q[:nx],   dU_h = g_q[nx:],   Lam_h = sym gS_h + A0^T Lam A0 + S~
 * traj, Sigma and the stage outputs have the BITS of gpk_propagate_mm_host[_multi].  The forward pass keeps the stages' queries,
 * Sigma_h, E[mu] and the clip indicators on the device; the backward pass recomputes each stage's set-up and row vectors (three
 * launches) ahead of the adjoint's four and keeps nothing of size N^2 or N R H: 6 H launches forward, 7 H backward, one upload,
 * ONE synchronisation.  Rollout r of a batch has the bits of that rollout alone; two calls agree bit for bit.
 * GPK_BAD_ARG (with a message, before any launch, the outputs untouched): the siblings' refusals, a seed with NaN or infinity, a
 * NULL gx, dx0 or (nu > 0) dU.                                                                                                  */
GPK_API int gpk_propagate_mm_grad_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                       double sf2, const double* y_mean, const double* y_std, const double* Kinv, int64_t Np,
                                       int64_t ldk, double kss, double floor_, int var_includes_noise, double noise,
                                       const double* x0, int x0_rows, const double* U, int u_rows, const double* lin,
                                       const double* Sigma0, int s_rows, const double* Q, int R, int H, double* traj, double* Sigma,
                                       double* mean, double* cov, double* xcov, const double* gx, const double* gS, double* dU,
                                       double* dx0, double* dSigma0);
GPK_API int gpk_propagate_mm_grad_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                             int D, const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                             const double* const* Kinv, int64_t Np, int64_t ldk, const double* kss, double floor_,
                                             int var_includes_noise, const double* noise, int nx, const int* coord,
                                             const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                             const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                             const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* cov,
                                             double* xcov, const double* gx, const double* gS, double* dU, double* dx0,
                                             double* dSigma0);

/* ... on the sparse posteriors.  The sparse posterior is the exact model's form over the m inducing inputs Z:
 *   mean(x) = y_mean + y_std k_u(x)^T alpha_u,     var_f(x) = sf2 - k_u(x)^T Q k_u(x),
 *   Q = Wuu^T Wuu - WSigma^T WSigma  ( = (Kuu + jitter_uu I)^-1 - Sigma~ )
 * so every closed form above carries over with (Z, alpha_u) as the rows and weights and Q where K^-1 stands: E[v_b] = kss_b -
 * sum_ij Q^b_ij L^bb_ij.  Q (mp x mp, the lower tiles, ld = mp) is formed on the device on the first of these calls after
 * gpk_sparse_finalize - two gpk_wtw products and one subtraction launch, one synchronisation - kept with the object and dropped
 * whenever the model is assembled again (gpk_sparse_finalize after more rows, the evaluations of gpk_sparse_eval[_z]).
 * kss = sf2, plus the model's noise level when var_includes_noise != 0; the clip of E[v] sits at 0.
 * gpk_sparse_moments: the finalised sparse object of h, P outputs sharing one L; nx <= D the width of the uncertain block.
 *   M <= 32 host queries Xq (M x D), Sq (M x nx x nx, the lower triangle is read; NULL: zero) -> mean (M x P), cov (M x P x P),
 *   xcov (M x P x D).
 * gpk_sparse_moments_multi: B <= 8 handles of finalised single-output models of equal m and D, each with its own Z, kernel, noise
 *   and normalisation, handle rules and scalers as gpk_sparse_propagate_multi -> mean (M x B), cov (M x B x B), xcov (M x B x D).
 * gpk_sparse_propagate_mm[_multi]: the horizon of gpk_propagate_mm_host[_multi] with the arguments of
 *   gpk_sparse_propagate[_multi] (nx = P in the single form) and (mean, cov, xcov) as the optional stage outputs, which have the
 *   BITS of gpk_sparse_moments[_multi] at the R Gaussian queries ([traj[h], U[h]], Sigma[h]).
 * Launches: those of the exact entries - five per batch of queries, 5 H and ONE synchronisation per horizon, the last of a stage
 *   under GPK_TIMED_PROPAGATE.  At the sparse sizes the pair launch has few tiles (m = 256: 10 lower 64 x 64 tiles per pair,
 *   m = 1024: 136) for 256 CUs, so its grid has a third dimension over groups of queries - as many groups as bring it to two
 *   workgroups per CU, one from 512 workgroups on (option "moments_query_groups": n >= 1 caps the count, 1 = no split; the exact
 *   entries take the same launch).  A slot is still summed by one workgroup over the same tiles in the same order: results do
 *   not depend on the split, are repeatable bit for bit, and query m has the bits of the same query served alone.  Launches of
 *   one group run the kernel without the dimension.  Measured (profiles/r28_exp_sparse_moments.log; D = 10, nx = 6, H = 25, one
 *   model with P = 6, R = 32 rollouts, wall time per horizon): m = 256 1.77 ms against 6.78 ms with one group, m = 1024 3.95
 *   against 6.80 ms, m = 4096 28.2 ms (one group either way); six models at m = 256 6.77 against 10.5 ms.  Registers and LDS of
 *   the pair kernel are unchanged: 135 (P = 1) .. 200 (P = 6) .. 256 (P >= 12) VGPRs, 46 .. 61 KB of LDS, no scratch.
 * GPK_BAD_ARG (with a message, before any launch - Q included - and with the outputs untouched): no finalised sparse model (in
 *   the batch: any handle), option small_path = 0, batched mode, models that disagree in m or D or have several outputs, B
 *   outside 1..8, M or R outside [1, 32], H outside [1, 256], nx or D above 16, nx > D, gpk_padded(m) > 16384, NaN or infinity
 *   in a host input, a scaler given by half, in_scale zero, a null pointer; the chains also: nx below the number of outputs,
 *   coord out of range or repeated, a wrong row count.
 *   Replaces: nothing in the reference; here, the first-order chain of gpk_sparse_propagate where the Taylor remainder matters. */
GPK_API int gpk_sparse_moments(gpk_handle h, int var_includes_noise, int nx, const double* Xq, const double* Sq, int M, double* mean,
                               double* cov, double* xcov);
GPK_API int gpk_sparse_moments_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                     const double* in_shift, const double* in_scale, const double* out_shift,
                                     const double* out_scale, const double* Xq, const double* Sq, int M, double* mean, double* cov,
                                     double* xcov);
GPK_API int gpk_sparse_propagate_mm(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U, int u_rows,
                                    const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H,
                                    double* traj, double* Sigma, double* mean, double* cov, double* xcov);
GPK_API int gpk_sparse_propagate_mm_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                          const int* coord, const double* in_shift, const double* in_scale,
                                          const double* out_shift, const double* out_scale, const double* x0, int x0_rows,
                                          const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                          const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* cov,
                                          double* xcov);
/* ... with the adjoint of the moments, on the same (Z, alpha_u, Q): the gradient of a horizon cost through the exact moments of the
 * sparse posteriors.  Q is a constant of the adjoint, as K^-1 is for the exact models.
 * gpk_sparse_moments_vjp[_multi]: the arguments of gpk_sparse_moments[_multi] followed by (gmean, gcov, gxcov, dXq, dSq) with the
 *   meaning, shapes and NULL rules of gpk_moments_vjp_host[_multi]: host seeds gmean (M x NO), gcov (M x NO x NO; (g + g^T) / 2 is
 *   used), gxcov (M x NO x D; columns >= nx ignored), NULL: zero; results dXq (M x D) and dSq (M x nx x nx, symmetric bit for bit)
 *   in raw units.  mean, cov and xcov have the BITS of gpk_sparse_moments[_multi].  Ten launches, one upload, five downloads, ONE
 *   synchronisation.
 * gpk_sparse_propagate_mm_grad[_multi]: the arguments of gpk_sparse_propagate_mm[_multi] followed by (gx, gS, dU, dx0, dSigma0) as
 *   gpk_propagate_mm_grad_host[_multi] has them: gx (H + 1, R, nx), gS (H + 1, R, nx, nx; NULL: zero), dU (R, H, nu; NULL only when
 *   nu = 0), dx0 (R, nx), dSigma0 (R, nx, nx; may be NULL).  traj, Sigma and the stage outputs have the BITS of
 *   gpk_sparse_propagate_mm[_multi].
 * Launches of the chain: at the sparse sizes a horizon is its launches and a stage's work block (the set-up results, the row
 *   vectors and the slots of the sums; about B^2 R mp 17 doubles and small terms) is a few megabytes, so these entries keep every
 *   stage's block in a region of its own - the tape - where H blocks fit option "moments_tape_mb" (default 1024 MiB, 0 = never; a
 *   memory cap): forward the five launches of gpk_sparse_propagate_mm per stage and no keep launch; backward four per stage, the
 *   set-up launch forming E[mu] and the clip indicators itself from the stage's slots in the keep launch's order
 *   (moments_grad_setup_taped_kernel: 0 bytes of scratch, no spill, no atomics) - 5 H + 4 H launches.  Beyond the cap: the
 *   6 H + 7 H sweep of the exact entries.  One upload and ONE synchronisation either way.  The tape moves buffers and fuses one
 *   reduction in its order; it reorders no sum: results are bit-identical with and without it, repeatable bit for bit, and rollout
 *   r has the bits of that rollout alone.  Option "gram_log": one line `GPKMT tape<0|1> h<H> stage<doubles> launches<n>` per
 *   chain, ahead of its GPKMM lines.  The exact entries do not ask for the tape.
 * GPK_BAD_ARG (with a message, before any launch - Q included - and with the outputs untouched): the refusals of the forward
 *   siblings, a seed with NaN or infinity, a NULL dXq or dSq, a NULL gx, dx0 or (nu > 0) dU.
 *   Replaces: nothing in the reference; here, the linearised gradient of gpk_sparse_propagate_grad where the controller optimises
 *   over the moment-matched horizon.                                                                                            */
GPK_API int gpk_sparse_moments_vjp(gpk_handle h, int var_includes_noise, int nx, const double* Xq, const double* Sq, int M,
                                   double* mean, double* cov, double* xcov, const double* gmean, const double* gcov,
                                   const double* gxcov, double* dXq, double* dSq);
GPK_API int gpk_sparse_moments_vjp_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                         const double* in_shift, const double* in_scale, const double* out_shift,
                                         const double* out_scale, const double* Xq, const double* Sq, int M, double* mean,
                                         double* cov, double* xcov, const double* gmean, const double* gcov, const double* gxcov,
                                         double* dXq, double* dSq);
GPK_API int gpk_sparse_propagate_mm_grad(gpk_handle h, int var_includes_noise, const double* x0, int x0_rows, const double* U,
                                         int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q, int R,
                                         int H, double* traj, double* Sigma, double* mean, double* cov, double* xcov,
                                         const double* gx, const double* gS, double* dU, double* dx0, double* dSigma0);
GPK_API int gpk_sparse_propagate_mm_grad_multi(gpk_handle h, int B, const gpk_handle* models, int var_includes_noise, int nx,
                                               const int* coord, const double* in_shift, const double* in_scale,
                                               const double* out_shift, const double* out_scale, const double* x0, int x0_rows,
                                               const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                               const double* Q, int R, int H, double* traj, double* Sigma, double* mean,
                                               double* cov, double* xcov, const double* gx, const double* gS, double* dU,
                                               double* dx0, double* dSigma0);

#ifdef __cplusplus
}
#endif
#endif /* GPK_H */
