// Composite entry points for B single-output models on shared inputs (the per-axis GPs of src/px4/gp_trainer.py:139-179):
// gpk_fit_batched / gpk_predict_batched / gpk_predict_batched_grad / gpk_predict_batched_cov / gpk_lml_batched.  The B
// factorisations, inverse factors and alpha solves run as ONE launch chain (gpk_batch_begin: every kernel of the chain gets
// a batch grid dimension); the Gram build, the LML reductions and the gradient reduction run once per model (their
// hyper-parameters differ).  Host pointers in, host pointers out; the device buffers are gpk_dev members of the model
// (gpk_compose.h, shared with gpk_model.hip and gpk_sparse.hip: buffer owner, query-panel loop, prologue pieces).
#include "gpk_compose.h"

struct gpk_bmodel {
  int B = 0, D = 0, n_ls = 0, normalize_y = 0;
  int64_t N = 0, Ne = 0, Np = 0;
  double jitter = 0.0;
  double ls[GPK_MAX_BATCH * GPK_MAX_D_PREDICT] = {0};      // one contiguous (B x D) block: model b's at ls + b * D
  double sf2[GPK_MAX_BATCH] = {0}, noise[GPK_MAX_BATCH] = {0}, y_mean[GPK_MAX_BATCH] = {0}, y_std[GPK_MAX_BATCH] = {0};
  double lml[GPK_MAX_BATCH] = {0};
  bool fitted = false;
  gpk_dev<double> X, Yn, alpha, alphaT, K, winv, W;
  const double *Xs[GPK_MAX_BATCH] = {nullptr}, *as[GPK_MAX_BATCH] = {nullptr}, *Ws[GPK_MAX_BATCH] = {nullptr};   // per model: X, alpha, W
  gpk_lml_scratch trial;         // gpk_lml_batched(thetas)
  gpk_dev<void> q, mean, work;
  gpk_dev<double> var;
  gpk_dev<void> cov;             // gpk_predict_batched_cov beyond 32 queries: one model's Sigma (Mp x Mp)
  size_t nn() const { return (size_t)Np * Np; }
  size_t tsz() const { return gpk_trtri_work(Np); }
  const double* ls_of(int b) const { return ls + b * D; }
  bool small(int64_t M) const { return M <= 32 && Np <= GPK_SMALL_MAX_NP; }      // the one-call route for all models
  void kss(int var_includes_noise, double* out) const {
    for (int b = 0; b < B; ++b) out[b] = gpk_kss(sf2[b], noise[b], var_includes_noise);
  }
};

namespace {

// alphaT[i][b] = alpha[b][i]: gpk_predict_mean_multi wants one column per model
__global__ void rows_to_cols_kernel(const double* __restrict__ rows, long long N, long long Ne, int B, double* __restrict__ cols) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < N * B) cols[i] = rows[(i % B) * Ne + i / B];
}

// out[m][b] = var[m] * s2  (column b of the M x B variance block)
__global__ void scale_var_col_kernel(const double* __restrict__ var, long long M, int B, int b, double s2, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < M) out[i * B + b] = var[i] * s2;
}

// out[m][b] = var[m] * s2 and out_g[m][b][d] = dvar[m][d] * s2  (column b of the M x B variance / M x B x D gradient blocks)
__global__ void scale_var_grad_col_kernel(const double* __restrict__ var, const double* __restrict__ dvar, long long M, int D, int B,
                                          int b, double s2, double* __restrict__ out, double* __restrict__ out_g) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * (D + 1)) return;
  const long long m = i / (D + 1);
  const int d = (int)(i - m * (D + 1));
  if (d < D) out_g[(m * B + b) * D + d] = dvar[m * D + d] * s2;
  else out[m * B + b] = var[m] * s2;
}

// K2 + W = L^-1 + K3 for all models in one launch chain; info[b] != 0: model b is not positive definite
int batched_chain(gpk_handle h, gpk_bmodel* m, double* T, int* info) {
  GPK_TRY(gpk_batch_begin(h, m->B));
  int rc = GPK_OK;
  const struct { const void* p; size_t stride; } bufs[] = {
      {m->K, m->nn() * 8}, {m->winv, (size_t)m->Np * GPK_TILE * 8}, {m->W, m->nn() * 8}, {T, m->tsz() * 8},
      {m->Yn, (size_t)m->Ne * 8}, {m->alpha, (size_t)m->Ne * 8}};
  for (const auto& b : bufs)
    if (rc == GPK_OK) rc = gpk_batch_buffer(h, b.p, (int64_t)b.stride);
  if (rc == GPK_OK) {
    rc = gpk_potrf(h, m->K, m->Np, m->Np, m->winv, info);
    if (rc == GPK_NOT_PD) rc = GPK_OK;            // per-model outcome is in info[]
  }
  if (rc == GPK_OK) rc = gpk_trtri(h, m->K, m->Np, m->Np, m->winv, m->W, m->Np, T);
  if (rc == GPK_OK) rc = gpk_potrs_inv(h, m->W, m->Np, m->Np, m->Yn, m->N, 1, m->alpha);
  (void)gpk_batch_end(h);
  return rc;
}

}  // namespace

void gpk_bmodel_free(gpk_handle h) {
  delete h->bmodel;
  h->bmodel = nullptr;
}

extern "C" int gpk_fit_batched(gpk_handle h, int B, const double* X, int64_t N, int D, const double* Y, const double* ls,
                               int n_ls, const double* sf2, const double* noise, double jitter, int normalize_y, int* info) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && Y && ls && sf2 && noise && info, "fit_batched: null pointer");
  GPK_REQUIRE(h, B >= 1 && B <= GPK_MAX_BATCH, "fit_batched: 1..8 models");
  GPK_REQUIRE(h, N >= 1 && D >= 1 && D <= GPK_MAX_D_PREDICT, "fit_batched: need N >= 1 and 1 <= D <= GPK_MAX_D_PREDICT");
  GPK_REQUIRE(h, n_ls == 1 || n_ls == D, "fit_batched: n_ls must be 1 (isotropic) or D (ARD)");
  GPK_REQUIRE(h, jitter >= 0.0, "fit_batched: jitter must be non-negative");
  GPK_REQUIRE(h, h->batch == 1, "composite calls are not available in batched mode");
  for (int b = 0; b < B; ++b) {
    GPK_REQUIRE(h, sf2[b] > 0.0 && noise[b] >= 0.0, "fit_batched: sf2 must be positive, noise non-negative");
    for (int d = 0; d < n_ls; ++d)
      GPK_REQUIRE(h, ls[b * n_ls + d] > 0.0 && std::isfinite(ls[b * n_ls + d]), "fit_batched: length-scales must be positive");
  }
  GPK_TRY(gpk_require_finite(h, X, N * D, "fit_batched", "X"));
  GPK_TRY(gpk_require_finite(h, Y, N * B, "fit_batched", "Y"));
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  gpk_bmodel_free(h);
  gpk_bmodel* m = h->bmodel = new gpk_bmodel();
  m->B = B; m->N = N; m->Ne = N + (N & 1); m->Np = gpk_padded(N); m->D = D; m->n_ls = n_ls; m->jitter = jitter;
  m->normalize_y = normalize_y ? 1 : 0;
  for (int b = 0; b < B; ++b) {
    for (int d = 0; d < D; ++d) m->ls[b * D + d] = ls[b * n_ls + (n_ls == 1 ? 0 : d)];
    m->sf2[b] = sf2[b]; m->noise[b] = noise[b];
  }
  // per-model rows (stride Ne: the batch strides must be multiples of 16 bytes, so odd N is padded by one entry)
  std::vector<double> yn((size_t)B * m->Ne, 0.0);
  for (int b = 0; b < B; ++b) gpk_normalize_column(Y + b, N, B, normalize_y, &m->y_mean[b], &m->y_std[b], yn.data() + (size_t)b * m->Ne, 1);
  GPK_TRY(m->X.alloc(h, (size_t)N * D));
  GPK_TRY(m->Yn.alloc(h, (size_t)B * m->Ne));
  GPK_TRY(m->alpha.alloc(h, (size_t)B * m->Ne));
  GPK_TRY(m->alphaT.alloc(h, (size_t)N * B));
  GPK_TRY(m->K.alloc(h, (size_t)B * m->nn()));
  GPK_TRY(m->winv.alloc(h, (size_t)B * m->Np * GPK_TILE));
  GPK_TRY(m->W.alloc(h, (size_t)B * m->nn()));
  for (int b = 0; b < B; ++b) { m->Xs[b] = m->X; m->as[b] = m->alpha + (size_t)b * m->Ne; m->Ws[b] = m->W + (size_t)b * m->nn(); }
  gpk_dev<double> T;
  GPK_TRY(T.alloc(h, (size_t)B * m->tsz()));
  GPK_CHECK_HIP(h, hipMemcpyAsync(m->X, X, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(m->Yn, yn.data(), yn.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; ++b)       // K1 per model
    GPK_TRY(gpk_gram(h, GPK_F64, m->X, N, D, m->ls_of(b), m->sf2[b], m->noise[b] + jitter, m->K + (size_t)b * m->nn(), m->Np));
  GPK_TRY(batched_chain(h, m, T, info));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));      // (T leaves scope)
  T.reset();
  bool all_pd = true;
  for (int b = 0; b < B; ++b) {
    if (info[b] != 0) { all_pd = false; m->lml[b] = -std::numeric_limits<double>::infinity(); continue; }
    double terms[2];
    GPK_TRY(gpk_lml_terms(h, m->K + (size_t)b * m->nn(), N, m->Np, m->Yn + (size_t)b * m->Ne, m->as[b], 1, terms));
    m->lml[b] = gpk_lml_value(terms[0], terms[1], N);
  }
  if (!all_pd) {
    h->err = "fit_batched: a model's matrix is not positive definite (see info[])";
    return GPK_NOT_PD;
  }
  const long long tot = (long long)N * B;
  hipLaunchKernelGGL(rows_to_cols_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, m->alpha.p, (long long)N,
                     (long long)m->Ne, B, m->alphaT.p);
  GPK_LAUNCH_CHECK(h);
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  m->fitted = true;
  return GPK_OK;
}

extern "C" int gpk_predict_batched(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var,
                                   int var_includes_noise) {
  if (!h) return GPK_BAD_ARG;
  gpk_bmodel* m = h->bmodel;
  GPK_REQUIRE(h, m && m->fitted, "predict_batched: no model (call gpk_fit_batched first)");
  GPK_REQUIRE(h, Xq && mean && M >= 1, "predict_batched: null pointer or empty batch");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int B = m->B, D = m->D;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "predict_batched", "Xq"));
  double kss[GPK_MAX_BATCH];
  m->kss(var_includes_noise, kss);
  const double floor_ = gpk_var_floor(var_includes_noise);
  // control-loop batches: one call, two launches for all models (src/px4/pretrained_gp.py:52-98)
  if (m->small(M)) {
    std::vector<double> mb((size_t)B * M), vb(var ? (size_t)B * M : 0);
    GPK_TRY(gpk_predict_host_multi(h, B, m->Xs, m->as, m->N, D, m->ls, m->sf2, m->y_mean, m->y_std, var ? m->Ws : nullptr, m->Np,
                                   m->Np, var ? kss : nullptr, floor_, Xq, M, mb.data(), var ? vb.data() : nullptr));
    gpk_interleave(mb.data(), B, M, 1, mean);
    if (var) {
      gpk_interleave(vb.data(), B, M, 1, var);
      for (int64_t i = 0; i < M; ++i)
        for (int b = 0; b < B; ++b) var[i * B + b] = var[i * B + b] * m->y_std[b] * m->y_std[b];
    }
    return GPK_OK;
  }
  const int64_t panel = gpk_panel_rows(4ull << 30, (size_t)m->Np * 8, M);
  GPK_TRY(m->q.reserve(h, (size_t)panel * D * 8));
  GPK_TRY(m->mean.reserve(h, (size_t)panel * B * 8));
  if (var) {
    GPK_TRY(m->work.reserve(h, (size_t)m->Np * panel * 8));
    GPK_TRY(m->var.reserve(h, (size_t)panel * 8 + (size_t)panel * B * 8));
  }
  double* d_varout = var ? m->var + panel : nullptr;
  return gpk_query_panels(h, Xq, M, (size_t)D * 8, panel, m->q, [&](int64_t m0, int64_t mc) -> int {
    GPK_TRY(gpk_predict_mean_multi(h, GPK_F64, m->X, m->alphaT, m->N, D, B, m->ls, m->sf2, m->y_mean, m->y_std, m->q, mc, m->mean));
    GPK_CHECK_HIP(h, hipMemcpyAsync(mean + (size_t)m0 * B, m->mean, (size_t)mc * B * 8, hipMemcpyDeviceToHost, h->stream));
    if (var) {
      for (int b = 0; b < B; ++b) {          // K* differs per model (its own length-scales): one variance launch each
        GPK_TRY(gpk_predict_var_inv(h, GPK_F64, m->X, m->N, D, m->ls_of(b), m->sf2[b], m->Ws[b], m->Np, m->Np, m->q, mc, kss[b],
                                    floor_, m->work, m->var));
        hipLaunchKernelGGL(scale_var_col_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, h->stream, m->var.p,
                           (long long)mc, B, b, m->y_std[b] * m->y_std[b], d_varout);
        GPK_LAUNCH_CHECK(h);
      }
      GPK_CHECK_HIP(h, hipMemcpyAsync(var + (size_t)m0 * B, d_varout, (size_t)mc * B * 8, hipMemcpyDeviceToHost, h->stream));
    }
    return GPK_OK;
  });
}

extern "C" int gpk_predict_batched_grad(gpk_handle h, const double* Xq, int64_t M, double* mean, double* var, double* dmean,
                                        double* dvar, int var_includes_noise) {
  if (!h) return GPK_BAD_ARG;
  gpk_bmodel* m = h->bmodel;
  GPK_REQUIRE(h, m && m->fitted, "predict_batched_grad: no model (call gpk_fit_batched first)");
  GPK_REQUIRE(h, Xq && mean && dmean && M >= 1, "predict_batched_grad: null pointer or empty batch");
  GPK_REQUIRE(h, (var == nullptr) == (dvar == nullptr), "predict_batched_grad: var and dvar come together (both or neither)");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int B = m->B, D = m->D;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "predict_batched_grad", "Xq"));
  double kss[GPK_MAX_BATCH];
  m->kss(var_includes_noise, kss);
  const double floor_ = gpk_var_floor(var_includes_noise);
  // control-loop batches: one call for all models, one launch (three with the variances)
  if (m->small(M)) {
    std::vector<double> mb((size_t)B * M), jb((size_t)B * M * D), vb(var ? (size_t)B * M : 0), gb(var ? (size_t)B * M * D : 0);
    GPK_TRY(gpk_predict_host_multi_grad(h, B, m->Xs, m->as, m->N, D, m->ls, m->sf2, m->y_mean, m->y_std, var ? m->Ws : nullptr, m->Np,
                                        m->Np, var ? kss : nullptr, floor_, Xq, M, mb.data(), var ? vb.data() : nullptr, jb.data(),
                                        var ? gb.data() : nullptr));
    gpk_interleave(mb.data(), B, M, 1, mean);
    gpk_interleave(jb.data(), B, M, D, dmean);
    if (var) {
      gpk_interleave(vb.data(), B, M, 1, var);
      gpk_interleave(gb.data(), B, M, D, dvar);
      for (int64_t i = 0; i < M; ++i)
        for (int b = 0; b < B; ++b) {
          const double s2 = m->y_std[b] * m->y_std[b];
          var[i * B + b] = var[i * B + b] * s2;
          for (int d = 0; d < D; ++d) dvar[(i * B + b) * D + d] = dvar[(i * B + b) * D + d] * s2;
        }
    }
    return GPK_OK;
  }
  // larger batches in query panels: the two fused launches for means and Jacobians of all models; per model the variance
  // gradient (its three Np x panel work panels within 6 GiB)
  const int64_t panel = gpk_panel_rows(6ull << 30, (size_t)3 * m->Np * 8, M);
  GPK_TRY(m->q.reserve(h, (size_t)panel * D * 8));
  GPK_TRY(m->mean.reserve(h, (size_t)panel * B * (D + 1) * 8));
  if (var) {
    GPK_TRY(m->work.reserve(h, (size_t)3 * m->Np * panel * 8));
    GPK_TRY(m->var.reserve(h, (size_t)panel * (D + 1) * 8 + (size_t)panel * B * (D + 1) * 8));
  }
  const double* dq = (const double*)m->q.p;
  double* d_mean = (double*)m->mean.p;
  double* d_dmean = d_mean + (size_t)panel * B;
  double* d_v1 = var ? m->var.p : nullptr;                             // one model: var (panel) | dvar (panel x D)
  double* d_g1 = var ? d_v1 + panel : nullptr;
  double* d_varout = var ? d_g1 + (size_t)panel * D : nullptr;         // (panel x B) | (panel x B x D)
  double* d_dvarout = var ? d_varout + (size_t)panel * B : nullptr;
  return gpk_query_panels(h, Xq, M, (size_t)D * 8, panel, m->q, [&](int64_t m0, int64_t mc) -> int {
    GPK_TRY(gpk_predict_mean_multi(h, GPK_F64, m->X, m->alphaT, m->N, D, B, m->ls, m->sf2, m->y_mean, m->y_std, dq, mc, d_mean));
    GPK_TRY(gpk_predict_mean_grad_multi(h, m->X, m->alphaT, m->N, D, B, m->ls, m->sf2, m->y_std, dq, mc, d_dmean));
    GPK_CHECK_HIP(h, hipMemcpyAsync(mean + (size_t)m0 * B, d_mean, (size_t)mc * B * 8, hipMemcpyDeviceToHost, h->stream));
    GPK_CHECK_HIP(h, hipMemcpyAsync(dmean + (size_t)m0 * B * D, d_dmean, (size_t)mc * B * D * 8, hipMemcpyDeviceToHost, h->stream));
    if (var) {
      for (int b = 0; b < B; ++b) {          // K*, W and the length-scales differ per model: one variance-gradient chain each
        GPK_TRY(gpk_predict_var_grad_inv(h, m->X, m->N, D, m->ls_of(b), m->sf2[b], m->Ws[b], m->Np, m->Np, dq, mc, kss[b], floor_,
                                         (double*)m->work.p, d_v1, d_g1));
        const long long tot = (long long)mc * (D + 1);
        hipLaunchKernelGGL(scale_var_grad_col_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, d_v1, d_g1,
                           (long long)mc, D, B, b, m->y_std[b] * m->y_std[b], d_varout, d_dvarout);
        GPK_LAUNCH_CHECK(h);
      }
      GPK_CHECK_HIP(h, hipMemcpyAsync(var + (size_t)m0 * B, d_varout, (size_t)mc * B * 8, hipMemcpyDeviceToHost, h->stream));
      GPK_CHECK_HIP(h, hipMemcpyAsync(dvar + (size_t)m0 * B * D, d_dvarout, (size_t)mc * B * D * 8, hipMemcpyDeviceToHost, h->stream));
    }
    return GPK_OK;
  });
}

extern "C" int gpk_predict_batched_hess(gpk_handle h, const double* Xq, int64_t M, double* mean, double* dmean, double* hess) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, hess != nullptr, "predict_batched_hess: hess is null");
  gpk_bmodel* m = h->bmodel;
  GPK_REQUIRE(h, m && m->fitted, "predict_batched_hess: no model (call gpk_fit_batched first)");
  GPK_REQUIRE(h, Xq && mean && dmean && M >= 1, "predict_batched_hess: null pointer or empty batch");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int B = m->B, D = m->D;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "predict_batched_hess", "Xq"));
  // control-loop batches: one call for all models
  if (m->small(M)) {
    std::vector<double> mb((size_t)B * M), jb((size_t)B * M * D), hb((size_t)B * M * D * D);
    GPK_TRY(gpk_predict_host_multi_hess(h, B, m->Xs, m->as, m->N, D, m->ls, m->sf2, m->y_mean, m->y_std, Xq, M, mb.data(), jb.data(),
                                        hb.data()));
    gpk_interleave(mb.data(), B, M, 1, mean);
    gpk_interleave(jb.data(), B, M, D, dmean);
    gpk_interleave(hb.data(), B, M, D * D, hess);
    return GPK_OK;
  }
  // larger batches in the query panels of gpk_predict_batched_grad: its two fused launches for means and Jacobians (their bits);
  // inside a panel the Hessians of all models in blocks of at most 64 MiB, one fused launch each
  const int64_t panel = gpk_panel_rows(6ull << 30, (size_t)3 * m->Np * 8, M);
  int64_t hrows = gpk_panel_rows(64ull << 20, (size_t)B * D * D * 8, M);
  if (hrows > panel) hrows = panel;
  const size_t nh1 = (size_t)hrows * D * D;
  GPK_TRY(m->q.reserve(h, (size_t)panel * D * 8));
  GPK_TRY(m->mean.reserve(h, ((size_t)panel * B * (D + 1) + (size_t)B * nh1) * 8));
  const double* dq = (const double*)m->q.p;
  double* d_mean = (double*)m->mean.p;
  double* d_dmean = d_mean + (size_t)panel * B;
  double* d_hess = d_dmean + (size_t)panel * B * D;      // (hrows x B x D x D)
  return gpk_query_panels(h, Xq, M, (size_t)D * 8, panel, m->q, [&](int64_t m0, int64_t mc) -> int {
    GPK_TRY(gpk_predict_mean_multi(h, GPK_F64, m->X, m->alphaT, m->N, D, B, m->ls, m->sf2, m->y_mean, m->y_std, dq, mc, d_mean));
    GPK_TRY(gpk_predict_mean_grad_multi(h, m->X, m->alphaT, m->N, D, B, m->ls, m->sf2, m->y_std, dq, mc, d_dmean));
    GPK_CHECK_HIP(h, hipMemcpyAsync(mean + (size_t)m0 * B, d_mean, (size_t)mc * B * 8, hipMemcpyDeviceToHost, h->stream));
    GPK_CHECK_HIP(h, hipMemcpyAsync(dmean + (size_t)m0 * B * D, d_dmean, (size_t)mc * B * D * 8, hipMemcpyDeviceToHost, h->stream));
    for (int64_t r0 = 0; r0 < mc; r0 += hrows) {
      const int64_t rc = mc - r0 < hrows ? mc - r0 : hrows;
      GPK_TRY(gpk_predict_mean_hess_multi(h, m->X, m->alphaT, m->N, D, B, m->ls, m->sf2, m->y_std, dq + r0 * D, rc, d_hess));
      GPK_CHECK_HIP(h, hipMemcpyAsync(hess + (size_t)(m0 + r0) * B * D * D, d_hess, (size_t)B * rc * D * D * 8, hipMemcpyDeviceToHost,
                                      h->stream));
    }
    return GPK_OK;
  });
}

extern "C" int gpk_predict_batched_cov(gpk_handle h, const double* Xq, int64_t M, double* mean, double* cov) {
  if (!h) return GPK_BAD_ARG;
  gpk_bmodel* m = h->bmodel;
  GPK_REQUIRE(h, m && m->fitted, "predict_batched_cov: no model (call gpk_fit_batched first)");
  GPK_REQUIRE(h, Xq && mean && cov && M >= 1 && M <= 16384, "predict_batched_cov: null pointer or M outside [1, 16384]");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  const int B = m->B, D = m->D;
  GPK_TRY(gpk_require_finite(h, Xq, M * D, "predict_batched_cov", "Xq"));
  const size_t nc = (size_t)M * M;
  if (m->small(M)) {
    // the horizon: one call, two launches for all models
    std::vector<double> mb((size_t)B * M);
    GPK_TRY(gpk_predict_host_multi_cov(h, B, m->Xs, m->as, m->N, D, m->ls, m->sf2, m->y_mean, m->y_std, m->Ws, m->Np, m->Np, m->noise,
                                       Xq, M, mb.data(), cov));
    gpk_interleave(mb.data(), B, M, 1, mean);
  } else {
    // larger batches: the fused mean launch, then per model V = W K*^T and Sigma (K*, W and the length-scales differ per
    // model); the work buffers are reused, the stream orders the models; one panel, one synchronisation
    const int64_t Mp = gpk_padded(M);
    GPK_TRY(m->q.reserve(h, (size_t)M * D * 8));
    GPK_TRY(m->mean.reserve(h, (size_t)M * B * 8));
    GPK_TRY(m->work.reserve(h, (size_t)m->Np * Mp * 8));
    GPK_TRY(m->cov.reserve(h, (size_t)Mp * Mp * 8));
    GPK_TRY(gpk_query_panels(h, Xq, M, (size_t)D * 8, M, m->q, [&](int64_t, int64_t) -> int {
      GPK_TRY(gpk_predict_mean_multi(h, GPK_F64, m->X, m->alphaT, m->N, D, B, m->ls, m->sf2, m->y_mean, m->y_std, m->q, M, m->mean));
      GPK_CHECK_HIP(h, hipMemcpyAsync(mean, m->mean, (size_t)M * B * 8, hipMemcpyDeviceToHost, h->stream));
      for (int b = 0; b < B; ++b) {
        GPK_TRY(gpk_predict_cov_inv(h, GPK_F64, m->X, m->N, D, m->ls_of(b), m->sf2[b], m->Ws[b], m->Np, m->Np, m->q, M, m->noise[b],
                                    m->work, (double*)m->cov.p, Mp));
        GPK_CHECK_HIP(h, hipMemcpy2DAsync(cov + b * nc, (size_t)M * sizeof(double), m->cov, (size_t)Mp * sizeof(double),
                                          (size_t)M * sizeof(double), (size_t)M, hipMemcpyDeviceToHost, h->stream));
      }
      return GPK_OK;
    }));
  }
  // model b: y_std[b]^2 Sigma_b (sklearn/_gpr.py:462-463)
  for (int b = 0; b < B; ++b) {
    const double s2 = m->y_std[b] * m->y_std[b];
    double* out = cov + b * nc;
    for (size_t i = 0; i < nc; ++i) out[i] = out[i] * s2;
  }
  return GPK_OK;
}

extern "C" int gpk_lml_batched(gpk_handle h, const double* thetas, int n_theta, double* lml, double* grad) {
  if (!h) return GPK_BAD_ARG;
  gpk_bmodel* m = h->bmodel;
  GPK_REQUIRE(h, m && m->fitted, "lml_batched: no model (call gpk_fit_batched first)");
  GPK_REQUIRE(h, lml, "lml_batched: null pointer");
  const int B = m->B, D = m->D;
  if (!thetas) {
    GPK_REQUIRE(h, !grad, "lml_batched: the gradient needs thetas");
    for (int b = 0; b < B; ++b) lml[b] = m->lml[b];
    return GPK_OK;
  }
  GPK_REQUIRE(h, n_theta == 2 || n_theta == D + 1, "lml_batched: each theta row holds log length-scale(s) and log noise");
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  double ls[GPK_MAX_BATCH * GPK_MAX_D_PREDICT], noise[GPK_MAX_BATCH];      // ls: (B x D)
  for (int b = 0; b < B; ++b) gpk_theta_to_hyper(thetas + b * n_theta, n_theta, D, ls + b * D, &noise[b]);
  gpk_lml_scratch& t = m->trial;
  GPK_TRY(t.ensure(h, (size_t)B * m->nn(), (size_t)B * m->tsz(), (size_t)B * m->Np * GPK_TILE, (size_t)B * m->Ne, grad != nullptr));
  for (int b = 0; b < B; ++b)
    GPK_TRY(gpk_gram(h, GPK_F64, m->X, m->N, D, ls + b * D, m->sf2[b], noise[b] + m->jitter, t.K + (size_t)b * m->nn(), m->Np));
  int info[GPK_MAX_BATCH] = {0};
  double terms[2 * GPK_MAX_BATCH], g[GPK_MAX_BATCH * (GPK_MAX_D_PREDICT + 2)];
  // factor, inverse factor, alpha, K^-1, terms and gradient passes of all B models: one chain, one synchronisation
  GPK_TRY(gpk_lml_chain_batched(h, B, m->X, m->N, D, ls, m->sf2, noise, m->Yn, m->Ne, t.K, m->Np, t.winv, t.W, t.T, m->tsz(), t.alpha,
                                grad ? t.Kinv.p : nullptr, terms, g, info));
  for (int b = 0; b < B; ++b) {
    if (info[b] != 0) {              // inside an optimiser: LML = -inf, zero gradient (_gpr.py:586-589)
      lml[b] = -std::numeric_limits<double>::infinity();
      if (grad) for (int i = 0; i < n_theta; ++i) grad[b * n_theta + i] = 0.0;
      continue;
    }
    lml[b] = gpk_lml_value(terms[2 * b], terms[2 * b + 1], m->N);
    if (grad) gpk_theta_grad(g + (size_t)b * (D + 2), n_theta, D, grad + (size_t)b * n_theta);
  }
  return GPK_OK;
}
