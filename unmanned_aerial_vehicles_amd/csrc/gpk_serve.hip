// One-call serving for the control loop: host queries in, host results out, one stream synchronisation per call.
//
//   gpk_predict_host, gpk_predict_host_multi             mean (+ variance)             of one model / of B per-axis models
//   gpk_predict_host_cov, gpk_predict_host_multi_cov     mean + covariance             of one model / of B per-axis models
//   gpk_predict_host_grad, gpk_predict_host_multi_grad   mean + Jacobian (+ variance + its gradient)
//
// The staging block is pinned, coherent host memory mapped into the device's address space: the kernels write their
// results straight into it (a few hundred bytes over PCIe) - no download command.  Small batches (<= 32 queries): the
// kernels read the queries from it as well (gpk_small.hip: one to three launches, no copy command).  Otherwise the
// queries go to HBM with one async copy (every workgroup re-reads them) ahead of the general chain.
//
// An entry checks its arguments, decides the route and calls one of gpk_serve_predict / gpk_serve_cov / gpk_serve_grad.  Those
// take a ServeModels (gpk_internal.h): the single-model entries are B = 1, the per-axis entries P = 1, both with one inverse
// factor; the sparse model's entries (gpk_sparse.hip) call the same three with two, for their small route.
#include "gpk_internal.h"

namespace {

// Grow the serving staging blocks (pinned, device-mapped host block; device work block) to at least these sizes.
int serve_reserve(gpk_handle h, size_t host_need, size_t dev_need) {
  if (host_need <= h->serve_host_bytes && dev_need <= h->serve_dev_bytes) return GPK_OK;
  GPK_CHECK_HIP(h, hipSetDevice(h->device));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  if (host_need > h->serve_host_bytes) {
    if (h->serve_host) GPK_CHECK_HIP(h, hipHostFree(h->serve_host));
    h->serve_host = nullptr; h->serve_host_bytes = 0;
    const size_t want = (host_need + 65535) & ~(size_t)65535;
    GPK_CHECK_HIP(h, hipHostMalloc(&h->serve_host, want, hipHostMallocMapped | hipHostMallocCoherent));
    h->serve_host_bytes = want;
  }
  if (dev_need > h->serve_dev_bytes) {
    if (h->serve_dev) GPK_CHECK_HIP(h, hipFree(h->serve_dev));
    h->serve_dev = nullptr; h->serve_dev_bytes = 0;
    const size_t want = (dev_need + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
    GPK_CHECK_HIP(h, hipMalloc(&h->serve_dev, want));
    h->serve_dev_bytes = want;
  }
  return GPK_OK;
}

// The staging of one call - the one place that knows the two blocks' layout:
//   pinned host block  [Xq | pad to 16 doubles][the outputs in the order they were named | pad to 16 doubles]
//   device block       [Xq | pad to 16 doubles][work]
// Use: out() for every output, begin(), the launches (after upload() if they read the queries from HBM), finish().
struct Serve {
  gpk_handle h;
  const double* Xq_host;
  size_t nxq, nq;                // doubles of queries; their slot (rounded up) in both blocks
  double *hq = nullptr, *dq = nullptr, *dwork = nullptr;   // set by begin(): queries in the pinned / the device block, work area
  struct Out { double* dst; double** at; size_t off, n; };
  Out outs[4];
  int nouts = 0;
  size_t nout = 0;

  Serve(gpk_handle h_, const double* Xq, int64_t M, int D)
      : h(h_), Xq_host(Xq), nxq((size_t)M * D), nq((nxq + 15) & ~(size_t)15) {}

  // The next output: n doubles.  begin() stores its address in the pinned block to *at; finish() copies it to dst
  // (dst null: not requested - the slot stays, nothing is copied).
  void out(double* dst, size_t n, double** at) {
    outs[nouts++] = Out{dst, at, nout, n};
    nout += n;
  }

  // Sizes the blocks for the named outputs and `work_doubles` of device work area (overwritten with NaN bytes under the
  // debug_fill option: whoever reads work must have written it) and places the queries in the pinned block.
  int begin(size_t work_doubles) {
    const size_t nout_pad = (nout + 15) & ~(size_t)15;
    GPK_TRY(serve_reserve(h, (nq + nout_pad) * sizeof(double), (nq + work_doubles) * sizeof(double)));
    hq = (double*)h->serve_host;
    dq = (double*)h->serve_dev;
    dwork = dq + nq;
    for (int i = 0; i < nouts; ++i) *outs[i].at = hq + nq + outs[i].off;
    if (h->debug_fill && work_doubles > 0)
      GPK_CHECK_HIP(h, hipMemsetAsync(dwork, 0xFF, work_doubles * sizeof(double), h->stream));
    memcpy(hq, Xq_host, nxq * sizeof(double));
    return GPK_OK;
  }

  // the queries to HBM (dq), for the general chain
  int upload() {
    GPK_CHECK_HIP(h, hipMemcpyAsync(dq, hq, nxq * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return GPK_OK;
  }

  // the call's one synchronisation, then every requested output to its caller
  int finish() {
    GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < nouts; ++i)
      if (outs[i].dst) memcpy(outs[i].dst, *outs[i].at, outs[i].n * sizeof(double));
    return GPK_OK;
  }
};

}  // namespace

// Mean (B, M, P) and, if var_host, the variance.  small: up to 32 queries the small-batch launches, 33..64 (one model, one
// factor) the same twice (4 launches instead of the general chain's 7); otherwise (one model) the general chain.
int gpk_serve_predict(gpk_handle h, const ServeModels& m, bool small, const double* Xq_host, int64_t M, double* mean_host,
                      double* var_host) {
  GPK_REQUIRE(h, small || m.F == 1, "serving: the general chain takes one inverse factor (the sparse model has panel routes of its own)");
  GPK_REQUIRE(h, small || m.B == 1, "serving: the general chain serves one model per call");
  GPK_REQUIRE(h, M <= GPK_SMALL_MAX_M || (m.B == 1 && m.F == 1), "serving: more than 32 queries go to one model with one factor");
  const int64_t Npad = gpk_padded(m.N), Mp = gpk_padded(M);
  const size_t nm = (size_t)m.B * M * m.P;
  ServeOut o{};
  Serve s(h, Xq_host, M, m.D);
  s.out(mean_host, nm, &o.mean);
  s.out(var_host, m.F == 2 ? nm : (size_t)m.B * M, &o.var);
  // work: the small-batch kernels' K* and shares, or the K* panel of the variance GEMM
  GPK_TRY(s.begin(small ? gpk_small_work_doubles(GPK_SMALL_PREDICT, Npad, m.B, M, m.D, m.P, m.F) : (var_host ? (size_t)Mp * Npad : 0)));
  if (small) {
    for (int64_t m0 = 0; m0 < M; m0 += GPK_SMALL_MAX_M) {
      const int64_t mc = M - m0 < GPK_SMALL_MAX_M ? M - m0 : GPK_SMALL_MAX_M;
      const ServeOut chunk{o.mean + m0 * m.P, var_host ? o.var + m0 : nullptr, nullptr, nullptr, nullptr};
      GPK_TRY(gpk_small_launch(h, GPK_SMALL_PREDICT, m, s.hq + m0 * m.D, mc, s.dwork, chunk));
    }
  } else {
    GPK_TRY(s.upload());
    GPK_TRY(gpk_predict_mean(h, GPK_F64, m.X[0], m.alpha[0], m.N, m.D, m.P, m.ls, m.sf2[0], m.y_mean, m.y_std, s.dq, M, o.mean));
    if (var_host)
      GPK_TRY(gpk_predict_var_inv(h, GPK_F64, m.X[0], m.N, m.D, m.ls, m.sf2[0], m.W[0][0], m.Np, m.ldw, s.dq, M, m.kss[0], m.floor_,
                                  s.dwork, o.var));
  }
  return s.finish();
}

// Mean (B, M, P) and covariance (B, M, M), m.noise[b] on model b's diagonal.  small: the two small-batch launches for all
// models, the covariances through the pinned block; otherwise the general blocks model by model: V (Np x Mp) and Sigma
// (Mp x Mp) in the work area (reused: the stream orders the models) and one strided download per model.
int gpk_serve_cov(gpk_handle h, const ServeModels& m, bool small, const double* Xq_host, int64_t M, double* mean_host,
                  double* cov_host) {
  GPK_REQUIRE(h, small || m.F == 1, "serving: the general chain takes one inverse factor (the sparse model has panel routes of its own)");
  const int64_t Mp = gpk_padded(M);
  const size_t nm = (size_t)M * m.P, nc = (size_t)M * M;       // per model
  ServeOut o{};
  Serve s(h, Xq_host, M, m.D);
  s.out(mean_host, m.B * nm, &o.mean);
  if (small) s.out(cov_host, m.B * nc, &o.cov);
  GPK_TRY(s.begin(small ? gpk_small_work_doubles(GPK_SMALL_COV, m.Np, m.B, M, m.D, m.P, m.F) : (size_t)m.Np * Mp + (size_t)Mp * Mp));
  if (small) {
    GPK_TRY(gpk_small_launch(h, GPK_SMALL_COV, m, s.hq, M, s.dwork, o));
  } else {
    double* dV = s.dwork;
    double* dcov = s.dwork + (size_t)m.Np * Mp;
    GPK_TRY(s.upload());
    for (int b = 0; b < m.B; ++b) {
      const double* ls = m.ls + b * m.D;
      GPK_TRY(gpk_predict_mean(h, GPK_F64, m.X[b], m.alpha[b], m.N, m.D, m.P, ls, m.sf2[b], m.y_mean + b * m.P, m.y_std + b * m.P,
                               s.dq, M, o.mean + b * nm));
      GPK_TRY(gpk_predict_cov_inv(h, GPK_F64, m.X[b], m.N, m.D, ls, m.sf2[b], m.W[0][b], m.Np, m.ldw, s.dq, M, m.noise[b], dV, dcov,
                                  Mp));
      GPK_CHECK_HIP(h, hipMemcpy2DAsync(cov_host + b * nc, (size_t)M * sizeof(double), dcov, (size_t)Mp * sizeof(double),
                                        (size_t)M * sizeof(double), (size_t)M, hipMemcpyDeviceToHost, h->stream));
    }
  }
  return s.finish();
}

// Mean (B, M, P) and its Jacobian (B, M, P, D); with var_host / dvar_host (both or neither) also the variance and its
// gradient (B, M, D).  small: all models in one launch, or three.  Otherwise the general building blocks, model by model,
// the variance gradient on query panels whose three Np x panel work panels stay within 6 GiB (DeviceGP.VAR_PANEL_BYTES).
int gpk_serve_grad(gpk_handle h, const ServeModels& m, bool small, const double* Xq_host, int64_t M, double* mean_host,
                   double* var_host, double* dmean_host, double* dvar_host) {
  GPK_REQUIRE(h, small || m.F == 1, "serving: the general chain takes one inverse factor (the sparse model has panel routes of its own)");
  const bool want_var = var_host != nullptr;
  const int64_t Npad = gpk_padded(m.N);
  int64_t panel = (int64_t)((6ull << 30) / ((size_t)3 * Npad * sizeof(double))) / GPK_TILE * GPK_TILE;
  if (panel < GPK_TILE) panel = GPK_TILE;
  if (panel > gpk_padded(M)) panel = gpk_padded(M);
  const size_t nm = (size_t)M * m.P, njm = nm * m.D, njv = (size_t)M * m.D;     // per model
  ServeOut o{};
  Serve s(h, Xq_host, M, m.D);
  s.out(mean_host, m.B * nm, &o.mean);
  s.out(var_host, m.F == 2 ? m.B * nm : (size_t)m.B * M, &o.var);
  s.out(dmean_host, m.B * njm, &o.dmean);
  s.out(dvar_host, m.B * njv, &o.dvar);
  GPK_TRY(s.begin(small ? gpk_small_work_doubles(GPK_SMALL_GRAD, Npad, m.B, M, m.D, m.P, m.F) : (want_var ? (size_t)3 * Npad * panel : 0)));
  if (small) {      // (the slots of var and dvar stay when they are not requested; nothing is written to them)
    const ServeOut req{o.mean, want_var ? o.var : nullptr, o.dmean, want_var ? o.dvar : nullptr, nullptr};
    GPK_TRY(gpk_small_launch(h, GPK_SMALL_GRAD, m, s.hq, M, s.dwork, req));
  } else {
    GPK_TRY(s.upload());
    for (int b = 0; b < m.B; ++b) {
      const double* ls = m.ls + b * m.D;
      GPK_TRY(gpk_predict_mean(h, GPK_F64, m.X[b], m.alpha[b], m.N, m.D, m.P, ls, m.sf2[b], m.y_mean + b * m.P, m.y_std + b * m.P,
                               s.dq, M, o.mean + b * nm));
      GPK_TRY(gpk_predict_mean_grad(h, m.X[b], m.alpha[b], m.N, m.D, m.P, ls, m.sf2[b], m.y_std + b * m.P, s.dq, M, o.dmean + b * njm));
      if (want_var)
        for (int64_t m0 = 0; m0 < M; m0 += panel) {
          const int64_t mc = M - m0 < panel ? M - m0 : panel;
          GPK_TRY(gpk_predict_var_grad_inv(h, m.X[b], m.N, m.D, ls, m.sf2[b], m.W[0][b], m.Np, m.ldw, s.dq + m0 * m.D, mc, m.kss[b],
                                           m.floor_, s.dwork, o.var + b * M + m0, o.dvar + b * njv + m0 * m.D));
        }
    }
  }
  return s.finish();
}

// Mean (B, M, P), its Jacobian (B, M, P, D) and its Hessian (B, M, P, D, D).  Mean and Jacobian exactly as gpk_serve_grad forms
// them without the variance, so they keep its bits.  small: GPK_SMALL_HESS - that one launch for all models, then
// small_hess_kernel, both reading the queries from the pinned block: two launches, no copy command.  Otherwise the general
// blocks, model by model, on the queries uploaded once.  Every refusal of the blocks is checked here first: nothing is launched
// for a call that fails.
int gpk_serve_hess(gpk_handle h, const ServeModels& m, bool small, const double* Xq_host, int64_t M, double* mean_host,
                   double* dmean_host, double* hess_host) {
  GPK_REQUIRE(h, hess_host != nullptr, "serving: hess is null");
  GPK_REQUIRE(h, m.D >= 1 && m.D <= GPK_MAX_D_PREDICT && m.P >= 1 && m.P <= GPK_MAX_P, "serving: D <= 16, P <= 16");
  for (int i = 0; i < m.B * m.D; ++i) GPK_REQUIRE(h, m.ls[i] > 0.0, "serving: length-scales must be positive");
  const int64_t Npad = gpk_padded(m.N);
  const size_t nm = (size_t)M * m.P, njm = nm * m.D, nh = njm * m.D;     // per model
  ServeOut o{};
  double* ohess = nullptr;
  Serve s(h, Xq_host, M, m.D);
  s.out(mean_host, m.B * nm, &o.mean);
  s.out(dmean_host, m.B * njm, &o.dmean);
  s.out(hess_host, m.B * nh, &ohess);
  GPK_TRY(s.begin(small ? gpk_small_work_doubles(GPK_SMALL_HESS, Npad, m.B, M, m.D, m.P, m.F) : 0));
  if (small) {      // two launches for all models, the queries read from the pinned block
    const ServeOut req{o.mean, nullptr, o.dmean, nullptr, nullptr, ohess};
    GPK_TRY(gpk_small_launch(h, GPK_SMALL_HESS, m, s.hq, M, s.dwork, req));
    return s.finish();
  }
  GPK_TRY(s.upload());
  for (int b = 0; b < m.B; ++b) {
    const double* ls = m.ls + b * m.D;
    GPK_TRY(gpk_predict_mean(h, GPK_F64, m.X[b], m.alpha[b], m.N, m.D, m.P, ls, m.sf2[b], m.y_mean + b * m.P, m.y_std + b * m.P,
                             s.dq, M, o.mean + b * nm));
    GPK_TRY(gpk_predict_mean_grad(h, m.X[b], m.alpha[b], m.N, m.D, m.P, ls, m.sf2[b], m.y_std + b * m.P, s.dq, M, o.dmean + b * njm));
    GPK_TRY(gpk_predict_mean_hess(h, m.X[b], m.alpha[b], m.N, m.D, m.P, ls, m.sf2[b], m.y_std + b * m.P, s.dq, M, ohess + b * nh));
  }
  return s.finish();
}

extern "C" int gpk_predict_host_hess(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P,
                                     const double* ls, double sf2, const double* y_mean, const double* y_std,
                                     const double* Xq_host, int64_t M, double* mean_host, double* dmean_host, double* hess_host) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, hess_host != nullptr, "predict_host_hess: hess is null");
  GPK_REQUIRE(h, X && alpha && ls && y_mean && y_std && Xq_host && mean_host && dmean_host, "predict_host_hess: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1 && M <= GPK_HOST_MAX_M, "predict_host_hess: M must be in [1, GPK_HOST_MAX_M]");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P, "predict_host_hess: D <= 16, P <= 16");
  GPK_REQUIRE(h, h->batch == 1, "predict_host_hess: not available in batched mode");
  const ServeModels m{1, P, 1, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, {nullptr, nullptr}, gpk_padded(N), gpk_padded(N), nullptr,
                      0.0, nullptr};
  return gpk_serve_hess(h, m, h->small_path && gpk_small_ok(gpk_padded(N), D, P, M), Xq_host, M, mean_host, dmean_host, hess_host);
}

extern "C" int gpk_predict_host_multi_hess(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                           int D, const double* ls, const double* sf2, const double* y_mean,
                                           const double* y_std, const double* Xq_host, int64_t M, double* mean_host,
                                           double* dmean_host, double* hess_host) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, hess_host != nullptr, "predict_host_multi_hess: hess is null");
  GPK_REQUIRE(h, X && alpha && ls && sf2 && y_mean && y_std && Xq_host && mean_host && dmean_host,
              "predict_host_multi_hess: null pointer");
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, "predict_host_multi_hess: 1..8 models");
  GPK_REQUIRE(h, N >= 1 && gpk_small_ok(gpk_padded(N), D, 1, M), "predict_host_multi_hess: needs M <= 32, D <= 16, N <= 16384");
  GPK_REQUIRE(h, h->batch == 1, "predict_host_multi_hess: not available in batched mode");
  for (int b = 0; b < B; ++b) GPK_REQUIRE(h, X[b] && alpha[b], "predict_host_multi_hess: null model pointer");
  // (option small_path = 0, the cross-check of the small-batch kernels: the general building blocks, model by model)
  const ServeModels m{B, 1, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, {nullptr, nullptr}, gpk_padded(N), gpk_padded(N), nullptr, 0.0,
                      nullptr};
  return gpk_serve_hess(h, m, h->small_path != 0, Xq_host, M, mean_host, dmean_host, hess_host);
}

extern "C" int gpk_predict_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P,
                                const double* ls, double sf2, const double* y_mean, const double* y_std,
                                const double* W, int64_t Np, int64_t ldw, double kss, double floor_,
                                const double* Xq_host, int64_t M, double* mean_host, double* var_host) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && ls && y_mean && y_std && Xq_host && mean_host, "predict_host: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1 && M <= GPK_HOST_MAX_M, "predict_host: M must be in [1, GPK_HOST_MAX_M]");
  GPK_REQUIRE(h, !var_host || (W && Np == gpk_padded(N) && ldw >= Np), "predict_host: variance needs the inverse factor");
  GPK_REQUIRE(h, h->batch == 1, "predict_host: not available in batched mode");
  const bool small = h->small_path && M <= 2 * GPK_SMALL_MAX_M &&
                     gpk_small_ok(gpk_padded(N), D, P, M < GPK_SMALL_MAX_M ? M : GPK_SMALL_MAX_M);
  const ServeModels m{1, P, 1, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, {&W, nullptr}, Np, ldw, &kss, floor_, nullptr};
  return gpk_serve_predict(h, m, small, Xq_host, M, mean_host, var_host);
}

extern "C" int gpk_predict_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                      int D, const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                      const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                      const double* Xq_host, int64_t M, double* mean_host, double* var_host) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && ls && sf2 && y_mean && y_std && Xq_host && mean_host, "predict_host_multi: null pointer");
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, "predict_host_multi: 1..8 models");
  GPK_REQUIRE(h, N >= 1 && gpk_small_ok(gpk_padded(N), D, 1, M), "predict_host_multi: needs M <= 32, D <= 16, N <= 16384");
  GPK_REQUIRE(h, !var_host || (W && kss && Np == gpk_padded(N) && ldw >= Np), "predict_host_multi: variance needs the inverse factors");
  GPK_REQUIRE(h, h->batch == 1, "predict_host_multi: not available in batched mode");
  // (no general route for the batch: the small-batch launches whatever the small_path option says)
  const ServeModels m{B, 1, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, {W, nullptr}, Np, ldw, kss, floor_, nullptr};
  return gpk_serve_predict(h, m, true, Xq_host, M, mean_host, var_host);
}

extern "C" int gpk_predict_host_cov(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P,
                                    const double* ls, double sf2, const double* y_mean, const double* y_std, const double* W,
                                    int64_t Np, int64_t ldw, double noise, const double* Xq_host, int64_t M, double* mean_host,
                                    double* cov_host) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && ls && y_mean && y_std && W && Xq_host && mean_host && cov_host, "predict_host_cov: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1 && M <= GPK_HOST_MAX_M, "predict_host_cov: M must be in [1, GPK_HOST_MAX_M]");
  GPK_REQUIRE(h, Np == gpk_padded(N) && ldw >= Np, "predict_host_cov: Np must equal gpk_padded(N), ldw >= Np");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P, "predict_host_cov: D <= 16, P <= 16");
  GPK_REQUIRE(h, h->batch == 1, "predict_host_cov: not available in batched mode");
  const ServeModels m{1, P, 1, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, {&W, nullptr}, Np, ldw, nullptr, 0.0, &noise};
  return gpk_serve_cov(h, m, h->small_path && gpk_small_ok(Np, D, P, M), Xq_host, M, mean_host, cov_host);
}

extern "C" int gpk_predict_host_multi_cov(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                          int D, const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                          const double* const* W, int64_t Np, int64_t ldw, const double* noise,
                                          const double* Xq_host, int64_t M, double* mean_host, double* cov_host) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && ls && sf2 && y_mean && y_std && W && noise && Xq_host && mean_host && cov_host,
              "predict_host_multi_cov: null pointer");
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, "predict_host_multi_cov: 1..8 models");
  GPK_REQUIRE(h, N >= 1 && gpk_small_ok(gpk_padded(N), D, 1, M), "predict_host_multi_cov: needs 1 <= M <= 32, D <= 16, N <= 16384");
  GPK_REQUIRE(h, Np == gpk_padded(N) && ldw >= Np, "predict_host_multi_cov: Np must equal gpk_padded(N), ldw >= Np");
  GPK_REQUIRE(h, h->batch == 1, "predict_host_multi_cov: not available in batched mode");
  for (int b = 0; b < B; ++b) GPK_REQUIRE(h, X[b] && alpha[b] && W[b], "predict_host_multi_cov: null model pointer");
  // (option small_path = 0, the cross-check of the small-batch kernels: the general building blocks, model by model)
  const ServeModels m{B, 1, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, {W, nullptr}, Np, ldw, nullptr, 0.0, noise};
  return gpk_serve_cov(h, m, h->small_path != 0, Xq_host, M, mean_host, cov_host);
}

extern "C" int gpk_predict_host_grad(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P,
                                     const double* ls, double sf2, const double* y_mean, const double* y_std, const double* W,
                                     int64_t Np, int64_t ldw, double kss, double floor_, const double* Xq_host, int64_t M,
                                     double* mean_host, double* var_host, double* dmean_host, double* dvar_host) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && ls && y_mean && y_std && Xq_host && mean_host && dmean_host, "predict_host_grad: null pointer");
  GPK_REQUIRE(h, N >= 1 && M >= 1 && M <= GPK_HOST_MAX_M, "predict_host_grad: M must be in [1, GPK_HOST_MAX_M]");
  GPK_REQUIRE(h, D >= 1 && D <= GPK_MAX_D_PREDICT && P >= 1 && P <= GPK_MAX_P, "predict_host_grad: D <= 16, P <= 16");
  GPK_REQUIRE(h, (var_host == nullptr) == (dvar_host == nullptr), "predict_host_grad: var and dvar come together (both or neither)");
  GPK_REQUIRE(h, !var_host || (W && Np == gpk_padded(N) && ldw >= Np), "predict_host_grad: the variance gradient needs the inverse factor");
  GPK_REQUIRE(h, h->batch == 1, "predict_host_grad: not available in batched mode");
  const ServeModels m{1, P, 1, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, {&W, nullptr}, Np, ldw, &kss, floor_, nullptr};
  return gpk_serve_grad(h, m, h->small_path && gpk_small_ok(gpk_padded(N), D, P, M), Xq_host, M, mean_host, var_host, dmean_host,
                    dvar_host);
}

extern "C" int gpk_predict_host_multi_grad(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N,
                                           int D, const double* ls, const double* sf2, const double* y_mean,
                                           const double* y_std, const double* const* W, int64_t Np, int64_t ldw,
                                           const double* kss, double floor_, const double* Xq_host, int64_t M,
                                           double* mean_host, double* var_host, double* dmean_host, double* dvar_host) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && ls && sf2 && y_mean && y_std && Xq_host && mean_host && dmean_host,
              "predict_host_multi_grad: null pointer");
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, "predict_host_multi_grad: 1..8 models");
  GPK_REQUIRE(h, N >= 1 && gpk_small_ok(gpk_padded(N), D, 1, M), "predict_host_multi_grad: needs M <= 32, D <= 16, N <= 16384");
  GPK_REQUIRE(h, (var_host == nullptr) == (dvar_host == nullptr),
              "predict_host_multi_grad: var and dvar come together (both or neither)");
  GPK_REQUIRE(h, !var_host || (W && kss && Np == gpk_padded(N) && ldw >= Np),
              "predict_host_multi_grad: the variance gradient needs the inverse factors");
  GPK_REQUIRE(h, h->batch == 1, "predict_host_multi_grad: not available in batched mode");
  for (int b = 0; b < B; ++b)
    GPK_REQUIRE(h, X[b] && alpha[b] && (!var_host || W[b]), "predict_host_multi_grad: null model pointer");
  // (option small_path = 0, the cross-check of the small-batch kernels: the general building blocks, model by model)
  const ServeModels m{B, 1, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, {W, nullptr}, Np, ldw, kss, floor_, nullptr};
  return gpk_serve_grad(h, m, h->small_path != 0, Xq_host, M, mean_host, var_host, dmean_host, dvar_host);
}
