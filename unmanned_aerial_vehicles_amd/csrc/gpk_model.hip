// Composite entry points of the libgpk C ABI: a whole GP model behind the handle - gpk_fit, gpk_predict, gpk_lml,
// gpk_export, gpk_import, gpk_model_release - for callers that are not Python.  Thin host code over
// the building blocks (K1 gpk_gram, K2 gpk_potrf, K3 gpk_potrs[_inv], K4 gpk_predict_mean[_mfma], K5
// gpk_predict_var_inv[_split], K6 gpk_lml_terms / gpk_wtw / gpk_lml_grad): the target normalisation
// (sklearn/gaussian_process/_gpr.py:271-282), the K1 -> K2 -> K3 sequencing (_gpr.py:343-364), the query panel loop
// and the optimiser objective (_gpr.py:537-652) that the Python host side (device.py, gpr.py) otherwise provides.
// Host pointers in, host pointers out; the device buffers are owned by the handle: every one is a gpk_dev (gpk_compose.h,
// which also holds the panel loop and the prologue pieces shared with gpk_bmodel.hip and gpk_sparse.hip).
#include "gpk_compose.h"

struct gpk_model {
  int64_t N = 0, Np = 0;
  int D = 0, P = 0, n_ls = 0, normalize_y = 0;
  double sf2 = 1.0, noise = 0.0, jitter = 0.0, lml = 0.0;
  double ls[GPK_MAX_D_PREDICT] = {0}, ls_in[GPK_MAX_D_PREDICT] = {0}, center[GPK_MAX_D_PREDICT] = {0};
  double y_mean[GPK_MAX_P] = {0}, y_std[GPK_MAX_P] = {0};
  bool fitted = false, mfma_mean_ok = false;
  // fp64 state
  gpk_dev<double> X, Yn, K, winv, W, alpha;
  bool has_W = false;
  // fp32 serving copies (built on the first fp32 predict)
  gpk_dev<float> Xf, alphaf;
  gpk_dev<uint32_t> W3;          // fp16 x 2 split of W in fragment order (gpk_split2_rows) ...
  gpk_dev<float> w_scales;       // ... and the power of two each 128-row block was scaled by
  gpk_dev<float> w_absmax;       // max |(float)W_ij| per 128-row block, left by gpk_trtri_absmax (the split's first pass)
  int f32_mean_ok = -1;          // fp32 serving gate on the mean (-1: not evaluated for the current alpha)
  gpk_lml_scratch trial;         // gpk_lml(theta)
  // query staging
  gpk_dev<void> q, mean, work, work3, q64;
  gpk_dev<double> var;
  gpk_dev<void> cov;             // gpk_predict_model_cov beyond GPK_HOST_MAX_M queries: Sigma (Mp x Mp)
};

namespace {

__global__ void to_float_kernel(const double* __restrict__ s, long long n, float* __restrict__ d) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) d[i] = (float)s[i];
}

// var_n[m] * y_std[p]^2 -> out[m][p]  (sklearn/_gpr.py:487-489: undo the normalisation of the variance)
template <typename T>
__global__ void scale_var_kernel(const double* __restrict__ var, long long M, int P, const double* __restrict__ ystd,
                                 T* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < M * P) { const double s = ystd[i % P]; out[i] = (T)(var[i / P] * s * s); }
}

// the fp32 matrix-core mean kernel expands |a - b|^2 around `center`; admissible while the largest scaled squared
// norm (exp2 units) stays below 64 (device.py MFMA_MEAN_R2_MAX; gpk.h gpk_predict_mean_mfma)
bool mfma_mean_admissible(const double* X, int64_t N, int D, int P, const double* ls, double* center) {
  for (int d = 0; d < D; ++d) {
    double s = 0.0;
    for (int64_t i = 0; i < N; ++i) s += X[i * D + d];
    center[d] = s / (double)N;
  }
  double r2 = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    double s = 0.0;
    for (int d = 0; d < D; ++d) { const double u = (X[i * D + d] - center[d]) / ls[d]; s += u * u; }
    if (s > r2) r2 = s;
  }
  return P <= 8 && 0.5 * 1.4426950408889634 * r2 <= 64.0;
}

// rows i_s = round(s (N - 1) / (S - 1)) of X (N x D) -> q (S x D)
__global__ void gather_rows_kernel(const double* __restrict__ X, long long N, int D, int S, double* __restrict__ q) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= S * D) return;
  const int s = e / D, d = e - s * D;
  const long long i = S > 1 ? (long long)llrint((double)s * (double)(N - 1) / (double)(S - 1)) : 0;
  q[e] = X[i * D + d];
}
__global__ void square_kernel(const double* __restrict__ a, long long n, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = a[i] * a[i];
}

// ---- fp32 serving gates (the rule of DeviceGP.predict_gated_dev, device.py) ------------------------------------------
// An fp32 kernel value carries the rounding of its exponent, so every term k*_j alpha_j of the mean is off by a few 1e-7
// of itself with random sign: mean error ~ c sqrt(sum_j (k*_j alpha_j)^2), c = 4.0e-7 for the matrix-core kernel and
// 9.0e-7 for the exact-difference kernel (worst query per batch over 41 random models: profiles/r02_fp32_gate_calibration.log).
// A2 = max_m sqrt(sum_j (k_mj alpha_j)^2) / max_m |mean_m| is measured on <= 1024 evenly spaced training rows (where it is
// largest) with two fp64 K4 launches - the second with the squared kernel (length-scales / sqrt 2, sf2^2) and squared
// weights - once per alpha; a model with c A2 above 1e-4 is served by the fp64 kernels.
// (round-4 calibration on batches up to 2^20 queries: profiles/r04_fp32_gate_calibration.log, device.py FP32_MEAN_ERR_PER_AMP)
constexpr double F32_MEAN_C_MFMA = 7.0e-7, F32_MEAN_C_VALU = 1.1e-6, F32_MEAN_TOL = 1e-4;
// fp32 variances below this fraction of the prior variance are recomputed in fp64 (their relative error is the absolute
// error of |W k*|^2 - up to 4e-5 kss - over the variance itself)
constexpr double F32_VAR_RECHECK_FRACTION = 1e-2;

int f32_mean_gate(gpk_handle h, gpk_model* m, bool* ok) {
  if (m->f32_mean_ok >= 0) { *ok = m->f32_mean_ok != 0; return GPK_OK; }
  const int D = m->D, P = m->P, S = (int)(m->N < 1024 ? m->N : 1024);
  gpk_dev<double> q, a2, o1, o2;
  if (q.alloc(h, (size_t)S * D) != GPK_OK || a2.alloc(h, (size_t)m->N * P) != GPK_OK || o1.alloc(h, (size_t)S * P) != GPK_OK ||
      o2.alloc(h, (size_t)S * P) != GPK_OK) {
    h->err = "fp32 mean gate: hipMalloc failed";
    return GPK_HIP_ERROR;
  }
  std::vector<double> h1((size_t)S * P), h2((size_t)S * P);
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((S * D + 255) / 256)), dim3(256), 0, h->stream, m->X.p,
                     (long long)m->N, D, S, q.p);
  const long long na = m->N * P;
  hipLaunchKernelGGL(square_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, h->stream, m->alpha.p, na, a2.p);
  double zeros[GPK_MAX_P] = {0}, ones[GPK_MAX_P], ls2[GPK_MAX_D_PREDICT];
  for (int p = 0; p < GPK_MAX_P; ++p) ones[p] = 1.0;
  for (int d = 0; d < D; ++d) ls2[d] = m->ls[d] / std::sqrt(2.0);
  GPK_TRY(gpk_predict_mean(h, GPK_F64, m->X, m->alpha, m->N, D, P, m->ls, m->sf2, zeros, ones, q, S, o1));
  GPK_TRY(gpk_predict_mean(h, GPK_F64, m->X, a2, m->N, D, P, ls2, m->sf2 * m->sf2, zeros, ones, q, S, o2));
  if (hipMemcpyAsync(h1.data(), o1, h1.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
      hipMemcpyAsync(h2.data(), o2, h2.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess) {
    h->err = "fp32 mean gate: copy failed";
    return GPK_HIP_ERROR;
  }
  double amp = 0.0;
  for (int p = 0; p < P; ++p) {
    double b = 0.0, a = 0.0;
    for (int s2 = 0; s2 < S; ++s2) {
      b = std::fmax(b, std::fabs(h1[(size_t)s2 * P + p]));
      a = std::fmax(a, h2[(size_t)s2 * P + p]);
    }
    amp = std::fmax(amp, std::sqrt(a) / std::fmax(b, 1e-300));
  }
  m->f32_mean_ok = ((m->mfma_mean_ok ? F32_MEAN_C_MFMA : F32_MEAN_C_VALU) * amp <= F32_MEAN_TOL) ? 1 : 0;
  *ok = m->f32_mean_ok != 0;
  return GPK_OK;
}

int set_hyper(gpk_handle h, gpk_model* m, const double* ls, int n_ls, double sf2, double noise, double jitter) {
  GPK_REQUIRE(h, ls && (n_ls == 1 || n_ls == m->D), "length-scales: n_ls must be 1 (isotropic) or D (ARD)");
  GPK_REQUIRE(h, sf2 > 0.0 && noise >= 0.0 && jitter >= 0.0, "sf2 must be positive, noise and jitter non-negative");
  for (int d = 0; d < m->D; ++d) {
    m->ls[d] = ls[n_ls == 1 ? 0 : d];
    GPK_REQUIRE(h, m->ls[d] > 0.0 && std::isfinite(m->ls[d]), "length-scales must be positive");
  }
  for (int d = 0; d < n_ls; ++d) m->ls_in[d] = ls[d];
  m->n_ls = n_ls; m->sf2 = sf2; m->noise = noise; m->jitter = jitter;
  return GPK_OK;
}

// W = L^-1 (one-off N^3/3 flops) - every later variance call and the alpha solve are then single GEMM launches
int ensure_W(gpk_handle h, gpk_model* m) {
  if (m->has_W) return GPK_OK;
  if (!m->W) GPK_TRY(m->W.alloc(h, (size_t)m->Np * m->Np));
  gpk_dev<double> T;
  GPK_TRY(T.alloc(h, gpk_trtri_work(m->Np)));
  if (!m->w_absmax && m->w_absmax.alloc(h, (size_t)(m->Np / 128)) != GPK_OK) {
    h->err = "fit: out of device memory";
    return GPK_HIP_ERROR;
  }
  GPK_TRY(gpk_trtri_absmax(h, m->K, m->Np, m->Np, m->winv, m->W, m->Np, T, m->w_absmax));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));      // (T leaves scope)
  m->has_W = true;
  m->W3.reset();            // the split form of the previous W
  return GPK_OK;
}

// fp32 serving form of K5: W as two fp16 parts per entry, straight from the fp64 inverse factor (no fp32 copy)
int split_W(gpk_handle h, gpk_model* m) {
  const size_t nblk = (size_t)(m->Np / 128);
  if (m->W3.alloc(h, (size_t)m->Np * m->Np) != GPK_OK || m->w_scales.alloc(h, nblk) != GPK_OK) {
    h->err = "predict: out of device memory for the split inverse factor";
    return GPK_HIP_ERROR;
  }
  // (the block maxima came out of gpk_trtri_absmax's epilogues: one pass over W)
  GPK_CHECK_HIP(h, hipMemcpyAsync(m->w_scales, m->w_absmax, nblk * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  GPK_TRY(gpk_split2_rows_f64_absmax(h, m->W, m->Np, m->Np, m->w_scales, m->W3));
  if (hipStreamSynchronize(h->stream) != hipSuccess) {
    h->err = "predict: split of the inverse factor failed";
    return GPK_HIP_ERROR;
  }
  return GPK_OK;
}

int new_model(gpk_handle h, int64_t N, int D, int P, gpk_model** out) {
  GPK_REQUIRE(h, N >= 1 && D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P,
              "need N >= 1, 1 <= D <= GPK_MAX_D_PREDICT, 1 <= P <= GPK_MAX_P");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  delete h->model;
  gpk_model* m = h->model = new gpk_model();
  m->N = N; m->Np = gpk_padded(N); m->D = D; m->P = P;
  GPK_TRY(m->X.alloc(h, (size_t)N * D));
  GPK_TRY(m->Yn.alloc(h, (size_t)N * P));
  GPK_TRY(m->alpha.alloc(h, (size_t)N * P));
  GPK_TRY(m->K.alloc(h, (size_t)m->Np * m->Np));
  GPK_TRY(m->winv.alloc(h, (size_t)m->Np * GPK_TILE));
  *out = m;
  return GPK_OK;
}

// up to this padded size W is formed at fit time (cheap); larger models form it on the first variance request
constexpr int64_t EAGER_W_NP = 32768;

}  // namespace

void gpk_model_free(gpk_handle h) {
  delete h->model;
  h->model = nullptr;
  gpk_bmodel_free(h);
  gpk_sparse_free(h);
}

extern "C" int gpk_model_release(gpk_handle h) {
  if (!h) return GPK_BAD_ARG;
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  gpk_model_free(h);
  return GPK_OK;
}

extern "C" int gpk_fit(gpk_handle h, const double* X, int64_t N, int D, const double* Y, int P, const double* ls,
                       int n_ls, double sf2, double noise, double jitter, int normalize_y) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Y, "fit: null pointer");
  gpk_model* m = nullptr;
  GPK_TRY(new_model(h, N, D, P, &m));
  GPK_TRY(set_hyper(h, m, ls, n_ls, sf2, noise, jitter));
  GPK_TRY(gpk_require_finite(h, X, N * D, "fit", "X"));
  GPK_TRY(gpk_require_finite(h, Y, N * P, "fit", "Y"));
  std::vector<double> yn((size_t)N * P);
  m->normalize_y = normalize_y ? 1 : 0;
  for (int p = 0; p < P; ++p) gpk_normalize_column(Y + p, N, P, normalize_y, &m->y_mean[p], &m->y_std[p], yn.data() + p, P);
  m->mfma_mean_ok = mfma_mean_admissible(X, N, D, P, m->ls, m->center);
  GPK_CHECK_HIP(h, hipMemcpyAsync(m->X, X, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(m->Yn, yn.data(), (size_t)N * P * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));      // (yn leaves scope)
  // K1 -> K2 -> K3   (_gpr.py:343-364); a non-positive-definite matrix is reported as GPK_NOT_PD (_gpr.py:350-358)
  GPK_TRY(gpk_gram(h, GPK_F64, m->X, N, D, m->ls, sf2, noise + jitter, m->K, m->Np));
  int info = 0;
  GPK_TRY(gpk_potrf(h, m->K, m->Np, m->Np, m->winv, &info));
  if (m->Np <= EAGER_W_NP) {
    GPK_TRY(ensure_W(h, m));
    GPK_TRY(gpk_potrs_inv(h, m->W, m->Np, m->Np, m->Yn, N, P, m->alpha));
  } else {
    GPK_TRY(gpk_potrs(h, m->K, m->Np, m->Np, m->winv, m->Yn, N, P, m->alpha));
  }
  double terms[1 + GPK_MAX_P];
  GPK_TRY(gpk_lml_terms(h, m->K, N, m->Np, m->Yn, m->alpha, P, terms));
  m->lml = 0.0;
  for (int p = 0; p < P; ++p) m->lml += gpk_lml_value(terms[0], terms[1 + p], N);
  m->fitted = true;
  return GPK_OK;
}

extern "C" int gpk_predict(gpk_handle h, const void* Xq, int64_t M, void* mean, void* var, int dtype,
                           int var_includes_noise) {
  if (!h) return GPK_BAD_ARG;
  gpk_model* m = h->model;
  GPK_REQUIRE(h, m && m->fitted, "predict: no model (call gpk_fit or gpk_import first)");
  GPK_REQUIRE(h, Xq && mean && M >= 1, "predict: null pointer or empty batch");
  GPK_REQUIRE(h, dtype == GPK_F32 || dtype == GPK_F64, "predict: bad dtype");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const bool f32 = dtype == GPK_F32;
  const size_t es = f32 ? 4 : 8;
  const int D = m->D, P = m->P;
  GPK_TRY(f32 ? gpk_require_finite(h, (const float*)Xq, M * D, "predict", "Xq")
              : gpk_require_finite(h, (const double*)Xq, M * D, "predict", "Xq"));
  const double kss = gpk_kss(m->sf2, m->noise, var_includes_noise), floor_ = gpk_var_floor(var_includes_noise);
  if (var) GPK_TRY(ensure_W(h, m));
  if (f32) {
    // fp32 serving is gated: a model whose fp32 mean would leave the stated 1e-4 is served by the fp64 kernels
    bool ok = true;
    GPK_TRY(f32_mean_gate(h, m, &ok));
    if (!ok) {
      std::vector<double> q64((size_t)M * D), m64((size_t)M * P), v64(var ? (size_t)M * P : 0);
      for (int64_t i = 0; i < M * D; ++i) q64[(size_t)i] = (double)((const float*)Xq)[i];
      GPK_TRY(gpk_predict(h, q64.data(), M, m64.data(), var ? v64.data() : nullptr, GPK_F64, var_includes_noise));
      for (int64_t i = 0; i < M * P; ++i) ((float*)mean)[i] = (float)m64[(size_t)i];
      if (var)
        for (int64_t i = 0; i < M * P; ++i) ((float*)var)[i] = (float)v64[(size_t)i];
      return GPK_OK;
    }
  }
  // control-loop batches, fp64: the one-call serving path (two launches up to 32 rows)
  if (!f32 && M <= 64 && (!var || m->Np <= GPK_SMALL_MAX_NP)) {
    std::vector<double> v1((size_t)M);
    GPK_TRY(gpk_predict_host(h, m->X, m->alpha, m->N, D, P, m->ls, m->sf2, m->y_mean, m->y_std, var ? m->W.p : nullptr,
                             m->Np, m->Np, kss, floor_, (const double*)Xq, M, (double*)mean, var ? v1.data() : nullptr));
    if (var)
      for (int64_t i = 0; i < M; ++i)
        for (int p = 0; p < P; ++p) ((double*)var)[i * P + p] = v1[(size_t)i] * m->y_std[p] * m->y_std[p];
    return GPK_OK;
  }
  if (f32 && !m->Xf) {
    GPK_TRY(m->Xf.alloc(h, (size_t)m->N * D));
    GPK_TRY(m->alphaf.alloc(h, (size_t)m->N * P));
    const long long nx = m->N * D, na = m->N * P;
    hipLaunchKernelGGL(to_float_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, h->stream, m->X.p, nx, m->Xf.p);
    hipLaunchKernelGGL(to_float_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, h->stream, m->alpha.p, na, m->alphaf.p);
    GPK_LAUNCH_CHECK(h);
  }
  if (f32 && var && !m->W3) {
    // all or nothing: a failure leaves no half-built operand behind for the next call to trust
    const int rc = split_W(h, m);
    if (rc != GPK_OK) { m->W3.reset(); m->w_scales.reset(); return rc; }
  }
  // panel loop: <= 16384 queries and <= 4 GiB of K* per panel
  const int64_t panel = gpk_panel_rows(4ull << 30, (size_t)m->Np * es, M);
  GPK_TRY(m->q.reserve(h, (size_t)panel * D * es));
  GPK_TRY(m->mean.reserve(h, (size_t)panel * P * es));
  if (var) {
    if (f32) GPK_TRY(m->work3.reserve(h, (size_t)m->Np * panel * 4));     // K* in split form only
    else GPK_TRY(m->work.reserve(h, (size_t)m->Np * panel * es));
    GPK_TRY(m->var.reserve(h, (size_t)panel * sizeof(double) + (size_t)panel * P * es + GPK_MAX_P * sizeof(double)));
  }
  double* d_ystd = nullptr;
  void* d_varout = nullptr;
  if (var) {
    d_ystd = m->var + panel;
    d_varout = (void*)(d_ystd + GPK_MAX_P);
    GPK_CHECK_HIP(h, hipMemcpyAsync(d_ystd, m->y_std, P * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  return gpk_query_panels(h, Xq, M, D * es, panel, m->q, [&](int64_t m0, int64_t mc) -> int {
    if (f32 && m->mfma_mean_ok)
      GPK_TRY(gpk_predict_mean_mfma(h, m->Xf, m->alphaf, m->N, D, P, m->ls, m->sf2, m->center, m->y_mean, m->y_std,
                                    (const float*)m->q.p, mc, (float*)m->mean.p));
    else
      GPK_TRY(gpk_predict_mean(h, dtype, f32 ? (const void*)m->Xf : (const void*)m->X,
                               f32 ? (const void*)m->alphaf : (const void*)m->alpha, m->N, D, P, m->ls, m->sf2, m->y_mean,
                               m->y_std, m->q, mc, m->mean));
    GPK_CHECK_HIP(h, hipMemcpyAsync((char*)mean + (size_t)m0 * P * es, m->mean, (size_t)mc * P * es, hipMemcpyDeviceToHost, h->stream));
    if (var) {
      if (f32) {
        GPK_TRY(gpk_predict_var_inv_split2(h, m->Xf, m->N, D, m->ls, m->sf2, m->W3, m->w_scales, m->Np, (const float*)m->q.p, mc,
                                           kss, floor_, m->work3, m->var));
        // fp32 variances that are a small fraction of the prior's are recomputed by the fp64 launch (F32_VAR_RECHECK_FRACTION)
        std::vector<double> vh((size_t)mc);
        GPK_CHECK_HIP(h, hipMemcpyAsync(vh.data(), m->var, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
        std::vector<int64_t> low;
        for (int64_t i = 0; i < mc; ++i)
          if (vh[(size_t)i] < F32_VAR_RECHECK_FRACTION * kss) low.push_back(i);
        for (size_t l0 = 0; l0 < low.size(); l0 += (size_t)panel) {
          const int64_t lc = (int64_t)std::min(low.size() - l0, (size_t)panel);
          std::vector<double> q64((size_t)lc * D), v2((size_t)lc);
          for (int64_t i = 0; i < lc; ++i)
            for (int d = 0; d < D; ++d) q64[(size_t)i * D + d] = (double)((const float*)Xq)[(size_t)(m0 + low[l0 + i]) * D + d];
          GPK_TRY(m->work.reserve(h, (size_t)m->Np * gpk_padded(lc) * sizeof(double)));
          GPK_TRY(m->q64.reserve(h, (size_t)lc * D * sizeof(double) + (size_t)gpk_padded(lc) * sizeof(double)));
          double* dq = (double*)m->q64.p;
          double* dv = dq + (size_t)lc * D;
          GPK_CHECK_HIP(h, hipMemcpyAsync(dq, q64.data(), q64.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
          GPK_TRY(gpk_predict_var_inv(h, GPK_F64, m->X, m->N, D, m->ls, m->sf2, m->W, m->Np, m->Np, dq, lc, kss, floor_,
                                      m->work, dv));
          GPK_CHECK_HIP(h, hipMemcpyAsync(v2.data(), dv, (size_t)lc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
          GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
          for (int64_t i = 0; i < lc; ++i) vh[(size_t)low[l0 + i]] = v2[(size_t)i];
        }
        for (int64_t i = 0; i < mc; ++i)      // undo the normalisation of the variance (sklearn/_gpr.py:487-489)
          for (int p = 0; p < P; ++p)
            ((float*)var)[(size_t)(m0 + i) * P + p] = (float)(vh[(size_t)i] * m->y_std[p] * m->y_std[p]);
      } else {
        GPK_TRY(gpk_predict_var_inv(h, GPK_F64, m->X, m->N, D, m->ls, m->sf2, m->W, m->Np, m->Np, m->q, mc, kss, floor_,
                                    m->work, m->var));
        const long long tot = mc * P;
        hipLaunchKernelGGL(scale_var_kernel<double>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, m->var.p,
                           (long long)mc, P, d_ystd, (double*)d_varout);
        GPK_LAUNCH_CHECK(h);
        GPK_CHECK_HIP(h, hipMemcpyAsync((char*)var + (size_t)m0 * P * es, d_varout, (size_t)mc * P * es, hipMemcpyDeviceToHost, h->stream));
      }
    }
    return GPK_OK;
  });
}

extern "C" int gpk_predict_model_cov(gpk_handle h, const double* Xq, int64_t M, double* mean, double* cov) {
  if (!h) return GPK_BAD_ARG;
  gpk_model* m = h->model;
  GPK_REQUIRE(h, m && m->fitted, "predict_model_cov: no model (call gpk_fit or gpk_import first)");
  GPK_REQUIRE(h, Xq && mean && cov && M >= 1 && M <= 16384, "predict_model_cov: null pointer or M outside [1, 16384]");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = m->D, P = m->P;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "predict_model_cov", "Xq"));
  GPK_TRY(ensure_W(h, m));
  std::vector<double> sig((size_t)M * M);
  if (M <= GPK_HOST_MAX_M) {
    GPK_TRY(gpk_predict_host_cov(h, m->X, m->alpha, m->N, D, P, m->ls, m->sf2, m->y_mean, m->y_std, m->W, m->Np, m->Np,
                                 m->noise, Xq, M, mean, sig.data()));
  } else {
    GPK_TRY(gpk_predict(h, Xq, M, mean, nullptr, GPK_F64, 1));
    const int64_t Mp = gpk_padded(M);
    GPK_TRY(m->q.reserve(h, (size_t)M * D * sizeof(double)));
    GPK_TRY(m->work.reserve(h, (size_t)m->Np * Mp * sizeof(double)));
    GPK_TRY(m->cov.reserve(h, (size_t)Mp * Mp * sizeof(double)));
    GPK_TRY(gpk_query_panels(h, Xq, M, D * sizeof(double), M, m->q, [&](int64_t, int64_t) -> int {      // one panel
      GPK_TRY(gpk_predict_cov_inv(h, GPK_F64, m->X, m->N, D, m->ls, m->sf2, m->W, m->Np, m->Np, m->q, M, m->noise, m->work,
                                  (double*)m->cov.p, Mp));
      GPK_CHECK_HIP(h, hipMemcpy2DAsync(sig.data(), (size_t)M * sizeof(double), m->cov, (size_t)Mp * sizeof(double),
                                        (size_t)M * sizeof(double), (size_t)M, hipMemcpyDeviceToHost, h->stream));
      return GPK_OK;
    }));
  }
  // output p: y_std[p]^2 Sigma (sklearn/_gpr.py:462-463)
  for (int p = 0; p < P; ++p) {
    const double s2 = m->y_std[p] * m->y_std[p];
    double* out = cov + (size_t)p * M * M;
    for (size_t i = 0; i < (size_t)M * M; ++i) out[i] = sig[i] * s2;
  }
  return GPK_OK;
}

extern "C" int gpk_predict_model_grad(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var, double* dmean,
                                      double* dvar, int var_includes_noise) {
  if (!h) return GPK_BAD_ARG;
  gpk_model* m = h->model;
  GPK_REQUIRE(h, m && m->fitted, "predict_model_grad: no model (call gpk_fit or gpk_import first)");
  GPK_REQUIRE(h, Xq && mean && dmean && M >= 1, "predict_model_grad: null pointer or empty batch");
  GPK_REQUIRE(h, (var == nullptr) == (dvar == nullptr), "predict_model_grad: var and dvar come together (both or neither)");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = m->D, P = m->P;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "predict_model_grad", "Xq"));
  const double kss = gpk_kss(m->sf2, m->noise, var_includes_noise), floor_ = gpk_var_floor(var_includes_noise);
  if (var) GPK_TRY(ensure_W(h, m));
  std::vector<double> v1, g1;
  for (int64_t m0 = 0; m0 < M; m0 += GPK_HOST_MAX_M) {
    const int64_t mc = M - m0 < GPK_HOST_MAX_M ? M - m0 : GPK_HOST_MAX_M;
    if (var) { v1.resize((size_t)mc); g1.resize((size_t)mc * D); }
    GPK_TRY(gpk_predict_host_grad(h, m->X, m->alpha, m->N, D, P, m->ls, m->sf2, m->y_mean, m->y_std, var ? m->W.p : nullptr, m->Np,
                                  m->Np, kss, floor_, Xq + m0 * D, mc, mean + m0 * P, var ? v1.data() : nullptr,
                                  dmean + m0 * P * D, var ? g1.data() : nullptr));
    if (var)      // undo the normalisation (sklearn/_gpr.py:487-489): output p carries y_std[p]^2
      for (int64_t i = 0; i < mc; ++i)
        for (int p = 0; p < P; ++p) {
          const double s2 = m->y_std[p] * m->y_std[p];
          var[(m0 + i) * P + p] = v1[(size_t)i] * s2;
          for (int d = 0; d < D; ++d) dvar[((m0 + i) * P + p) * D + d] = g1[(size_t)i * D + d] * s2;
        }
  }
  return GPK_OK;
}

extern "C" int gpk_predict_model_hess(gpk_handle h, const double* Xq, int64_t M, double* mean, double* dmean, double* hess) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, hess != nullptr, "predict_model_hess: hess is null");
  gpk_model* m = h->model;
  GPK_REQUIRE(h, m && m->fitted, "predict_model_hess: no model (call gpk_fit or gpk_import first)");
  GPK_REQUIRE(h, Xq && mean && dmean && M >= 1, "predict_model_hess: null pointer or empty batch");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = m->D, P = m->P;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "predict_model_hess", "Xq"));
  // query blocks whose Hessians stay within 32 MiB of the pinned block: a multiple of 32 rows, at most GPK_HOST_MAX_M
  int64_t rows = (int64_t)((32u << 20) / ((size_t)P * D * D * sizeof(double))) / 32 * 32;
  if (rows > GPK_HOST_MAX_M) rows = GPK_HOST_MAX_M;
  if (rows < 32) rows = 32;
  for (int64_t m0 = 0; m0 < M; m0 += rows) {
    const int64_t mc = M - m0 < rows ? M - m0 : rows;
    GPK_TRY(gpk_predict_host_hess(h, m->X, m->alpha, m->N, D, P, m->ls, m->sf2, m->y_mean, m->y_std, Xq + m0 * D, mc, mean + m0 * P,
                                  dmean + m0 * P * D, hess + m0 * P * D * D));
  }
  return GPK_OK;
}

extern "C" int gpk_lml(gpk_handle h, const double* theta, int n_theta, double* lml, double* grad) {
  if (!h) return GPK_BAD_ARG;
  gpk_model* m = h->model;
  GPK_REQUIRE(h, m && m->fitted, "lml: no model (call gpk_fit or gpk_import first)");
  GPK_REQUIRE(h, lml, "lml: null pointer");
  if (!theta) {                      // the fitted model's own value (_gpr.py:560-563)
    GPK_REQUIRE(h, !grad, "lml: the gradient needs theta");
    *lml = m->lml;
    return GPK_OK;
  }
  GPK_REQUIRE(h, m->normalize_y != -1, "lml(theta): an imported model does not carry the training targets");
  // theta = log [ls (1 value: isotropic, or D values: ARD), noise]; sf2 and jitter stay as fitted
  GPK_REQUIRE(h, n_theta == 2 || n_theta == m->D + 1, "lml: theta must hold log length-scale(s) and log noise");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int D = m->D, P = m->P;
  double ls[GPK_MAX_D_PREDICT], noise;
  gpk_theta_to_hyper(theta, n_theta, D, ls, &noise);
  gpk_lml_scratch& t = m->trial;
  GPK_TRY(t.ensure(h, (size_t)m->Np * m->Np, gpk_trtri_work(m->Np), (size_t)m->Np * GPK_TILE, (size_t)m->N * P, grad != nullptr));
  // the whole evaluation as one chain of launches with one synchronisation (gpk_lml_eval)
  int info = 0;
  double terms[1 + GPK_MAX_P], g[GPK_MAX_D_PREDICT + 2];
  const int rc = gpk_lml_eval(h, m->X, m->N, D, ls, m->sf2, noise + m->jitter, noise, m->Yn, P, t.K, m->Np, t.winv, t.W, t.T,
                              t.alpha, grad ? t.Kinv.p : nullptr, terms, grad ? g : nullptr, &info);
  if (rc == GPK_NOT_PD) {            // inside an optimiser: LML = -inf, zero gradient (_gpr.py:586-589)
    *lml = -std::numeric_limits<double>::infinity();
    if (grad) for (int i = 0; i < n_theta; ++i) grad[i] = 0.0;
    return GPK_OK;
  }
  GPK_TRY(rc);
  double v = 0.0;
  for (int p = 0; p < P; ++p) v += gpk_lml_value(terms[0], terms[1 + p], m->N);
  *lml = v;
  if (grad) gpk_theta_grad(g, n_theta, D, grad);
  return GPK_OK;
}

extern "C" int gpk_export(gpk_handle h, int64_t* N, int* D, int* P, double* L, double* alpha, double* y_mean,
                          double* y_std, double* lml) {
  if (!h) return GPK_BAD_ARG;
  gpk_model* m = h->model;
  GPK_REQUIRE(h, m && m->fitted, "export: no model");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  if (N) *N = m->N;
  if (D) *D = m->D;
  if (P) *P = m->P;
  if (L) {      // the lower factor, N x N row-major, zeros above the diagonal (what scikit-learn keeps as L_)
    GPK_CHECK_HIP(h, hipMemcpy2DAsync(L, (size_t)m->N * sizeof(double), m->K, (size_t)m->Np * sizeof(double),
                                      (size_t)m->N * sizeof(double), (size_t)m->N, hipMemcpyDeviceToHost, h->stream));
    GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < m->N; ++i)
      for (int64_t j = i + 1; j < m->N; ++j) L[i * m->N + j] = 0.0;
  }
  if (alpha) GPK_CHECK_HIP(h, hipMemcpyAsync(alpha, m->alpha, (size_t)m->N * m->P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  for (int p = 0; p < m->P; ++p) {
    if (y_mean) y_mean[p] = m->y_mean[p];
    if (y_std) y_std[p] = m->y_std[p];
  }
  if (lml) *lml = m->lml;
  return GPK_OK;
}

extern "C" int gpk_import(gpk_handle h, const double* X, int64_t N, int D, const double* L, const double* alpha, int P,
                          const double* ls, int n_ls, double sf2, double noise, const double* y_mean, const double* y_std) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && L && alpha && y_mean && y_std, "import: null pointer");
  gpk_model* m = nullptr;
  GPK_TRY(new_model(h, N, D, P, &m));
  GPK_TRY(set_hyper(h, m, ls, n_ls, sf2, noise, 0.0));
  for (int p = 0; p < P; ++p) { m->y_mean[p] = y_mean[p]; m->y_std[p] = y_std[p]; }
  m->mfma_mean_ok = mfma_mean_admissible(X, N, D, P, m->ls, m->center);
  GPK_CHECK_HIP(h, hipMemcpyAsync(m->X, X, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(m->alpha, alpha, (size_t)N * P * sizeof(double), hipMemcpyHostToDevice, h->stream));
  // the padded factor [L 0; 0 I]; Yn is not part of a stored model: Yn = (L L^T) alpha is not needed for prediction
  // (gpk_lml on an imported model is refused below)
  GPK_CHECK_HIP(h, hipMemsetAsync(m->K, 0, (size_t)m->Np * m->Np * sizeof(double), h->stream));
  GPK_CHECK_HIP(h, hipMemcpy2DAsync(m->K, (size_t)m->Np * sizeof(double), L, (size_t)N * sizeof(double),
                                    (size_t)N * sizeof(double), (size_t)N, hipMemcpyHostToDevice, h->stream));
  if (m->Np > N) {
    std::vector<double> ones((size_t)(m->Np - N), 1.0);
    GPK_CHECK_HIP(h, hipMemcpy2DAsync(m->K + N * m->Np + N, (size_t)(m->Np + 1) * sizeof(double), ones.data(), sizeof(double),
                                      sizeof(double), (size_t)(m->Np - N), hipMemcpyHostToDevice, h->stream));
    GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  }
  GPK_TRY(gpk_leaf_inverses(h, m->K, m->Np, m->Np, m->winv));
  if (m->Np <= EAGER_W_NP) GPK_TRY(ensure_W(h, m));
  // Yn = K alpha = L (L^T alpha) is recovered lazily only if gpk_lml is asked for: not supported on imported models
  GPK_CHECK_HIP(h, hipMemsetAsync(m->Yn, 0, (size_t)N * P * sizeof(double), h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  m->lml = std::numeric_limits<double>::quiet_NaN();
  m->normalize_y = -1;               // unknown: marks an imported model (gpk_lml(theta) needs the training targets)
  m->fitted = true;
  return GPK_OK;
}
