// What the composite entry points (gpk_model.hip, gpk_bmodel.hip, gpk_sparse.hip: a whole model behind the handle) share:
// the owner of a device buffer, the query-panel loop and the pieces of their prologues.  Header-only host code.
#pragma once
#include <cmath>
#include <limits>

#include "gpk_internal.h"

// ---- the owner of one device buffer ---------------------------------------------------------------------------------------
// A pointer and its size in bytes; hipFree in the destructor, no copies.  A model is a struct of these (freeing it is
// `delete`), a temporary is a local (every return frees it).  Both ways of filling it honour the debug_fill option: the bytes
// asked for are overwritten with 0xFF (NaN) on the stream at EVERY request, so whoever reads them must have written them.
template <typename T>
struct gpk_dev {
  T* p = nullptr;
  size_t bytes = 0;
  gpk_dev() = default;
  gpk_dev(const gpk_dev&) = delete;
  gpk_dev& operator=(const gpk_dev&) = delete;
  ~gpk_dev() { reset(); }
  operator T*() const { return p; }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // exactly `count` elements (whatever was held is freed first)
  int alloc(gpk_handle h, size_t count) {
    reset();
    GPK_CHECK_HIP(h, hipMalloc((void**)&p, count * sizeof(T)));
    bytes = count * sizeof(T);
    if (h->debug_fill && bytes) GPK_CHECK_HIP(h, hipMemsetAsync(p, 0xFF, bytes, h->stream));
    return GPK_OK;
  }
  // grow-only staging: at least `need` bytes; the stream is drained before a block that launches may still use is replaced
  int reserve(gpk_handle h, size_t need) {
    if (need > bytes) {
      GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
      reset();
      GPK_CHECK_HIP(h, hipMalloc((void**)&p, need));
      bytes = need;
    }
    if (h->debug_fill && need) GPK_CHECK_HIP(h, hipMemsetAsync(p, 0xFF, need, h->stream));
    return GPK_OK;
  }
};

// scratch of an LML evaluation at trial hyper-parameters: a second factorisation that leaves the fitted one alone
// (nn: entries of K / W / K^-1, tsz: of gpk_trtri's work area, nwinv: of the tile inverses, nalpha: of alpha - all problems of a batch)
struct gpk_lml_scratch {
  gpk_dev<double> K, W, Kinv, T, winv, alpha;
  int ensure(gpk_handle h, size_t nn, size_t tsz, size_t nwinv, size_t nalpha, bool want_Kinv) {
    if (!alpha) {      // (the last of the five: an allocation that failed half-way is taken up again)
      GPK_TRY(K.alloc(h, nn));
      GPK_TRY(W.alloc(h, nn));
      GPK_TRY(T.alloc(h, tsz));
      GPK_TRY(winv.alloc(h, nwinv));
      GPK_TRY(alpha.alloc(h, nalpha));
    }
    if (want_Kinv && !Kinv) GPK_TRY(Kinv.alloc(h, nn));
    return GPK_OK;
  }
};

inline size_t gpk_trtri_work(int64_t Np) { return (size_t)(Np / 2 + 128) * (Np / 2 + 128); }   // doubles (gpk.h, gpk_trtri)

// ---- M host queries through a panel of at most R rows -------------------------------------------------------------------
// R: the rows that `budget` bytes hold at `row_bytes` each, in whole tiles, within [128, 16384] and gpk_padded(M)
inline int64_t gpk_panel_rows(size_t budget, size_t row_bytes, int64_t M) {
  int64_t panel = (int64_t)(budget / row_bytes) / GPK_TILE * GPK_TILE;
  if (panel > 16384) panel = 16384;
  if (panel < GPK_TILE) panel = GPK_TILE;
  if (panel > gpk_padded(M)) panel = gpk_padded(M);
  return panel;
}
// Per panel: rows [m0, m0 + mc) of Xq (`row_bytes` each: D values of 4 or 8 bytes) go up to dq, body(m0, mc) issues the
// launches and the result copies, one synchronisation ends the panel (the staging blocks are reused by the next one).
template <typename Body>
int gpk_query_panels(gpk_handle h, const void* Xq, int64_t M, size_t row_bytes, int64_t panel, void* dq, Body&& body) {
  for (int64_t m0 = 0; m0 < M; m0 += panel) {
    const int64_t mc = M - m0 < panel ? M - m0 : panel;
    GPK_CHECK_HIP(h, hipMemcpyAsync(dq, (const char*)Xq + (size_t)m0 * row_bytes, (size_t)mc * row_bytes, hipMemcpyHostToDevice, h->stream));
    GPK_TRY(body(m0, mc));
    GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  }
  return GPK_OK;
}

// ---- prologue pieces ------------------------------------------------------------------------------------------------------
// "<entry>: <name> contains NaN or infinity" unless all n values of the host array are finite
template <typename T>
int gpk_require_finite(gpk_handle h, const T* a, int64_t n, const char* entry, const char* name) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite((double)a[i])) {
      h->err = std::string("bad argument: ") + entry + ": " + name + " contains NaN or infinity";
      return GPK_BAD_ARG;
    }
  return GPK_OK;
}

// the prior variance k** and the clip of the posterior variance: sklearn surface k** = sf2 + noise (Sum.diag), clipped at 0;
// package surface k** = sf2, floored at 1e-10
inline double gpk_kss(double sf2, double noise, int var_includes_noise) { return sf2 + (var_includes_noise ? noise : 0.0); }
inline double gpk_var_floor(int var_includes_noise) { return var_includes_noise ? 0.0 : 1e-10; }

// target normalisation of one output column (sklearn/gaussian_process/_gpr.py:271-282): population std, a (numerically)
// zero std counts as 1; out[i * so] = (Y[i * sy] - mean) / std.  Without `normalize`: mean 0, std 1.
inline void gpk_normalize_column(const double* Y, int64_t N, int64_t sy, int normalize, double* mean_out, double* std_out,
                                 double* out, int64_t so) {
  double mean = 0.0, std_ = 1.0;
  if (normalize) {
    for (int64_t i = 0; i < N; ++i) mean += Y[i * sy];
    mean /= (double)N;
    double v = 0.0;
    for (int64_t i = 0; i < N; ++i) { const double d = Y[i * sy] - mean; v += d * d; }
    std_ = std::sqrt(v / (double)N);
    if (std_ < 10.0 * std::numeric_limits<double>::epsilon()) std_ = 1.0;
  }
  *mean_out = mean; *std_out = std_;
  for (int64_t i = 0; i < N; ++i) out[i * so] = (Y[i * sy] - mean) / std_;
}

// log marginal likelihood of one output from gpk_lml_terms' sums: logdet = sum log diag L, quad = y^T alpha
inline double gpk_lml_value(double logdet, double quad, int64_t N) {
  return -0.5 * quad - logdet - 0.5 * (double)N * std::log(2.0 * M_PI);
}
// theta = log [length-scale (1 value: isotropic, or D values: ARD), noise] -> ls[0 .. D), noise
inline void gpk_theta_to_hyper(const double* theta, int n_theta, int D, double* ls, double* noise) {
  const int nl = n_theta - 1;
  for (int d = 0; d < D; ++d) ls[d] = std::exp(theta[nl == 1 ? 0 : d]);
  *noise = std::exp(theta[nl]);
}
// gpk_lml_grad's sums g = [d/dlog ls_0 .. ls_{D-1}, d/dlog noise, ..] -> the gradient in theta's layout (isotropic: the
// length-scale entries add up, kernels.py:1574-1576)
inline void gpk_theta_grad(const double* g, int n_theta, int D, double* grad) {
  const int nl = n_theta - 1;
  if (nl == 1) { double s = 0.0; for (int d = 0; d < D; ++d) s += g[d]; grad[0] = s; }
  else for (int d = 0; d < D; ++d) grad[d] = g[d];
  grad[nl] = g[D];
}

// (B, M, K) as the one-call entries return it -> (M, B, K) as the per-axis batch returns it
inline void gpk_interleave(const double* src, int B, int64_t M, int K, double* dst) {
  for (int64_t i = 0; i < M; ++i)
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < K; ++k) dst[((size_t)i * B + b) * K + k] = src[((size_t)b * M + i) * K + k];
}
