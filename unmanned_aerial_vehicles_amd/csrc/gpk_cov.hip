// Posterior covariance of a query batch (sklearn/gaussian_process/_gpr.py:454-469):
//
//   Sigma = K(Xq, Xq) + noise I - V^T V,   V = L^-1 K*^T   (Np x Mp, fp64; rows >= N and columns >= M are zero)
//
// V comes from the existing pieces - through the explicit inverse factor W = L^-1 (the cross-Gram panel and one tile
// GEMM with the plain store, W's zero upper triangle skipped: N^2 M flops as the variance launch) or through the blocked
// triangular solve - and Sigma from ONE symmetric tile GEMM over the lower 128 x 128 tiles of the Mp x Mp output (N M^2
// flops) whose epilogue (gpk_gemm.hip, epilogue 3) forms the prior term from the scaled queries, subtracts, and stores
// every tile and its transpose.  Up to 32 queries the one-call serving entry takes the two small-batch launches instead
// (gpk_small.hip: small_cross_mean_kernel + small_cov_kernel).
#include "gpk_internal.h"

namespace {

struct LsInv { double v[16]; };

// U[m][d] = Xq[m][d] / ls[d]: the queries in length-scale units (divided first, as scikit-learn's RBF does)
__global__ void scale_queries_kernel(const double* __restrict__ Xq, long long M, int D, LsInv ls, double* __restrict__ U) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < M * D) U[e] = Xq[e] / ls.v[e % D];
}

}  // namespace

// Sigma (Mp x ldc) from V (Np x Mp, ld Mp; VA == VB for the exact model) and the queries: the scaled queries go to the
// handle's scratch
int gpk_cov_from_v(gpk_handle h, const double* VA, const double* VB, int64_t Np, const double* Xq, int64_t M, int D,
                   const double* ls, double sf2, double noise, double* cov, int64_t ldc) {
  GPK_REQUIRE(h, D >= 1 && D <= 16, "predict_cov: D must be in [1, 16]");
  const int64_t Mp = gpk_padded(M);
  LsInv l{};
  for (int d = 0; d < 16; ++d) l.v[d] = 1.0;
  for (int d = 0; d < D; ++d) {
    GPK_REQUIRE(h, ls[d] > 0.0, "length-scales must be positive");
    l.v[d] = ls[d];
  }
  void* u = nullptr;
  GPK_TRY(gpk_scratch(h, (size_t)M * D * sizeof(double), &u));
  hipLaunchKernelGGL(scale_queries_kernel, dim3((unsigned)((M * D + 255) / 256)), dim3(256), 0, h->stream, Xq, (long long)M, D,
                     l, (double*)u);
  GPK_LAUNCH_CHECK(h);
  GemmArgs g = gemm_args(VA, Mp, 1, VB, Mp, 1, cov, ldc, (int)Mp, (int)Mp, (int)Np, 1.0, 0.0);
  g.lower_only = 1;
  g.epilogue = 3;
  g.cov_q = (const double*)u;
  g.cov_sf2 = sf2;
  g.cov_noise = noise;
  g.cov_d = D;
  g.cov_m = (int)M;
  gpk_time_begin(h, GPK_TIMED_COV);
  const int rc = gpk_gemm(h, GPK_F64, g);
  gpk_time_end(h);
  return rc;
}

namespace {

int cov_args_ok(gpk_handle h, int dtype, int64_t N, int64_t Np, int64_t M, int64_t ldc) {
  GPK_REQUIRE(h, dtype == GPK_F64, "predict_cov: fp64 only (there is no fp32 covariance)");
  GPK_REQUIRE(h, N >= 1 && M >= 1 && Np == gpk_padded(N), "predict_cov: Np must equal gpk_padded(N)");
  GPK_REQUIRE(h, M <= 65536 && ldc >= gpk_padded(M) && ldc % 2 == 0, "predict_cov: ldc must be >= gpk_padded(M) (even)");
  GPK_REQUIRE(h, h->batch == 1, "predict_cov: not available in batched mode");
  return GPK_OK;
}

}  // namespace

extern "C" int gpk_predict_cov_inv(gpk_handle h, int dtype, const void* X, int64_t N, int D, const double* ls, double sf2,
                                   const void* W, int64_t Np, int64_t ldw, const void* Xq, int64_t M, double noise, void* work,
                                   double* cov, int64_t ldc) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && ls && W && Xq && work && cov, "predict_cov_inv: null pointer");
  GPK_TRY(cov_args_ok(h, dtype, N, Np, M, ldc));
  GPK_REQUIRE(h, ldw >= Np, "predict_cov_inv: ldw must be >= Np");
  const int64_t Mp = gpk_padded(M);
  // Kq (Mp x Np, query-major, k contiguous) = k(Xq, X) in the scratch, zero in the padding
  void* kq = nullptr;
  GPK_TRY(gpk_scratch(h, (size_t)Mp * Np * sizeof(double), &kq));
  GPK_TRY(gpk_cross_gram_t(h, GPK_F64, Xq, M, X, N, D, ls, sf2, kq, Np));
  // V = W Kq^T (Np x Mp) with the plain store; W lower: tile row tm needs k < (tm + 1) * 128
  GemmArgs g = gemm_args(W, ldw, 0, kq, Np, 0, work, Mp, (int)Np, (int)Mp, (int)Np, 1.0, 0.0);
  g.ke0 = GPK_TILE;
  g.ke_row = GPK_TILE;
  g.k_super = 1;            // W is zero right of the diagonal for GPK_ZERO_BAND_TILES - 1 tiles (gpk_trtri)
  g.heavy_first = 1;
  GPK_TRY(gpk_gemm(h, GPK_F64, g));
  return gpk_cov_from_v(h, (const double*)work, (const double*)work, Np, (const double*)Xq, M, D, ls, sf2, noise, cov, ldc);
}

extern "C" int gpk_predict_cov(gpk_handle h, int dtype, const void* X, int64_t N, int D, const double* ls, double sf2,
                               const void* L, int64_t Np, int64_t ldl, const void* winv, const void* Xq, int64_t M, double noise,
                               void* work, double* cov, int64_t ldc) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && ls && L && winv && Xq && work && cov, "predict_cov: null pointer");
  GPK_TRY(cov_args_ok(h, dtype, N, Np, M, ldc));
  const int64_t Mp = gpk_padded(M);
  // B = K*^T (Np x Mp), V = L^-1 B in place (the variance path's solve)
  GPK_TRY(gpk_cross_gram_t(h, GPK_F64, X, N, Xq, M, D, ls, sf2, work, Mp));
  GPK_TRY(gpk_trsm_lower_left(h, GPK_F64, L, Np, ldl, winv, work, Mp, Mp));
  return gpk_cov_from_v(h, (const double*)work, (const double*)work, Np, (const double*)Xq, M, D, ls, sf2, noise, cov, ldc);
}
