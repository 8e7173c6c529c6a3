// Horizon propagation (K11): the posterior's own mean rollout with the linearised state covariance, one call per horizon.
//
//   q = [x_h, u_h],  z = (q - in_shift) / in_scale
//   x_{h+1}     = x_h + lin q + sum_b e_coord[b] mu_b(z)
//   A_h         = I + lin[:, :nx] + sum_b e_coord[b] J_b[:nx]              J_b = d mu_b / d q (raw units)
//   Sigma_{h+1} = A_h Sigma_h A_h^T + sum_b v_b(z) e_coord[b] e_coord[b]^T + Q
//
// Every stage's query is the previous stage's result, so a stage is three launches in stream order and nothing else: the two
// small-batch launches of GPK_SMALL_JACVAR (gpk_small.hip: mean + Jacobian + variance of the R query rows, the bits of
// gpk_predict_host[_multi]_grad at those rows) and propagate_advance_kernel below, which composes the stage and writes the next
// stage's scaled query rows where its first launch reads them.  The state (x, Sigma), the queries, the stage results and the
// horizon's outputs stay in one device block; ONE upload before the chain ([x | Sigma | q | lin | Q | U] as one block), up to five
// downloads and ONE stream synchronisation after it.  The caller's arrays are ordinary (pageable) host memory: the runtime stages
// those copies and may wait on them by itself; nothing waits between the stages.
//
// ONE skeleton carries every chain (declared in gpk_internal.h beside Horizon, defined below):
//   gpk_horizon_check    R, H, the row counts, the null pointers and NaN / infinity in the horizon's host arrays
//   HorizonBlock         the device block, sized and carved by the same take() calls (gpk_horizon_carve runs them twice): head(),
//                        the chain's own buffers, outputs()
//   gpk_horizon_pack     the upload's head on the host;  gpk_horizon_upload  slot 0 of traj / Sigma and the one copy in
//   gpk_horizon_stage    StageView of stage s: its controls and the next stage's, x, S, the next queries, the output slots
//   gpk_horizon_finish   the downloads and the one synchronisation
// and the composing launch of every chain builds its stage from the helpers of gpk_horizon.h.  What each chain adds:
//   linear, order 1      propagate_forward on GPK_SMALL_JACVAR (gpk_propagate_run; 3 launches per stage).  It serves the exact
//                        models' entries below and the sparse models' in gpk_sparse.hip (two inverse factors per model: the
//                        stage's variance arrives final and in another layout, which PropK's strides describe).
//   linear, order 2      the trace launch ahead of the advance and its shares, tr St and c of every stage in the block (4)
//   gradient             (Horizon::grad; order 1) propagate_forward on the three launches of GPK_SMALL_GRAD - the variance gradient
//                        comes with them, mean, Jacobian and variance keep their bits - with every stage's queries, Jacobians and
//                        variance gradients kept in the block, then per stage, backwards, the Hessian-vector launch
//                        (small_hvp_kernel, gpk_small.hip) and propagate_adjoint_kernel below; the seeds ride behind the head in
//                        the one upload, three more downloads (propagate_run_grad; 6)
//   moment               (gpk_moments.hip, gpk_mm_chain) the four moment launches and moments_finish_kernel as the composing launch,
//                        the moment work area in the block (5)
#include "gpk_horizon.h"

namespace {

constexpr int PROP_MAX_NX = GPK_PROP_MAX_NX, PROP_MAX_D = GPK_PROP_MAX_D;
constexpr int PROP_MAX_GROUPS = 64;      // workgroups per model of the trace launch (gpk_small_trace_groups) at most

// One workgroup per rollout r, thread (i, j) = (tid >> 4, tid & 15).  Sequential, fixed-order sums; Sigma in LDS; the lower
// triangle of T A^T is formed and mirrored, so Sigma is symmetric bit for bit.  x and S are the rollout's state, updated in
// place (this workgroup alone touches row r of either); qnext: the next stage's scaled queries (R x D), null at the last stage.
//
// SECOND (propagate_advance2_kernel, order 2): the stage's trace launch (small_hess_trace_kernel, gpk_small.hip) has left `groups`
// shares of T = sum_j k* alpha delta^T St delta and S = sum_j k* alpha per (rollout, output) and tr St per (rollout, model).  The
// kernel adds them in workgroup order, forms c_o = y_std[o] (T - tr St S) / 2 = tr(H_o Sigma_h) / 2 and adds c to xn LAST, as one
// addition to the finished first-order value.  A, Sigma and the stage's outputs are the first-order kernel's, bit for bit.
struct Prop2 {
  const double* shares;              // groups x (NO R) x 2, entry e = o * so + r * sm
  const double* trs;                 // tr St of (rollout r, output o) at [o * tro + r]
  int groups, tro;
  double ystd[16];
  double* ocorr;                     // this stage's c (R x NO), or null
};

template <bool SECOND>
__device__ __forceinline__ void propagate_advance_body(const PropK& k, const StageView& v, int R, const double* __restrict__ smean,
                                                       const double* __restrict__ svar, const double* __restrict__ sjac,
                                                       const Prop2* p2) {
  __shared__ double A[16][17], Sg[16][17], T[16][17], J[16][17];
  __shared__ double q[16], mu[16], vv[16], xn[16];
  [[maybe_unused]] double (*cc)[16] = nullptr;
  if constexpr (SECOND) {
    __shared__ double cc_s[16];
    cc = &cc_s;
  }
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, r = blockIdx.x;
  const int nx = k.nx, D = k.D, NO = k.NO;
  stage_load(v, nx, D, r, tid, q, Sg);
  if (tid < NO) {
    const double var = svar[tid * k.vo + r * k.vm];
    mu[tid] = smean[tid * k.so + r * k.sm];
    vv[tid] = (k.add_noise ? var + k.noise[tid] : var) * k.ystd2[tid];
  }
  if constexpr (SECOND) {
    // the shares of output i: thread (i, j) fetches those of workgroups j, j + 16, .. (all loads in flight together), thread
    // (i, 0) adds them in workgroup order
    __shared__ double sh[2][16][PROP_MAX_GROUPS + 1];
    const long long E = (long long)NO * R, e = i * k.so + r * k.sm;
    if (i < NO)
      for (int g = j; g < p2->groups; g += 16) {
        sh[0][i][g] = p2->shares[(g * E + e) * 2];
        sh[1][i][g] = p2->shares[(g * E + e) * 2 + 1];
      }
    __syncthreads();
    if (tid < NO) {
      double t = 0.0, s = 0.0;
      for (int g = 0; g < p2->groups; ++g) {
        t += sh[0][tid][g];
        s += sh[1][tid][g];
      }
      (*cc)[tid] = 0.5 * (p2->ystd[tid] * (t - p2->trs[tid * p2->tro + r] * s));
    }
  }
  if (i < NO && j < D) {
    const double g = sjac[(long long)(i * k.so + r * k.sm) * D + j];
    J[i][j] = k.scaled ? g / k.in_scale[j] : g;
  }
  __syncthreads();
  if (i < nx && j < nx) {
    const int o = k.model_of[i];
    double a = (i == j ? 1.0 : 0.0) + v.lin[i * D + j];
    if (o >= 0) a += J[o][j];
    A[i][j] = a;
  }
  stage_mean(v, k.model_of, nx, D, tid, q, mu, xn);
  __syncthreads();
  stage_left(nx, tid, A, Sg, T);
  __syncthreads();
  stage_right(v, nx, r, tid, T, A, [&](double s, int a, int b) {
    const int o = k.model_of[a];
    return a == b && o >= 0 ? s + vv[o] : s;
  });
  if constexpr (SECOND) {
    if (tid < nx) {
      const int o = k.model_of[tid];
      if (o >= 0) xn[tid] += (*cc)[o];
    }
    if (p2->ocorr && tid < NO) p2->ocorr[(long long)r * NO + tid] = (*cc)[tid];
  }
  stage_store(v, k.scaled, k.in_shift, k.in_scale, nx, D, r, tid, xn);
  if (tid < NO) {
    if (v.out[0]) v.out[0][(long long)r * NO + tid] = mu[tid];
    if (v.out[1]) v.out[1][(long long)r * NO + tid] = vv[tid];
  }
  if (v.out[2] && i < NO && j < D) v.out[2][((long long)r * NO + i) * D + j] = J[i][j];
}

__global__ __launch_bounds__(256) void propagate_advance_kernel(PropK k, StageView v, int R, const double* __restrict__ smean,
                                                                const double* __restrict__ svar, const double* __restrict__ sjac) {
  propagate_advance_body<false>(k, v, R, smean, svar, sjac, nullptr);
}
__global__ __launch_bounds__(256) void propagate_advance2_kernel(PropK k, StageView v, int R, const double* __restrict__ smean,
                                                                 const double* __restrict__ svar, const double* __restrict__ sjac,
                                                                 Prop2 p2) {
  propagate_advance_body<true>(k, v, R, smean, svar, sjac, &p2);
}

// The backward stage h of the gradient of a horizon cost (order 1), after the stage's Hessian-vector launch (small_hvp_kernel,
// gpk_small.hip).  With lam = dl/dx_{h+1} and Lam = dl/dSigma_{h+1} (symmetric) as the stage above left them:
//   F    = [I 0] + lin + sum_b e_c J_b                                  (nx x D; its first nx columns are A_h, the advance kernel's bits)
//   g_q  = F^T lam + sum_b Lam[c_b][c_b] grad v_b + 2 sum_b H_b w_b     (w_b: row c_b of Lam A_h Sigma_h; the launch before left the
//                                                                       workgroups' shares of H_b w_b, added here in workgroup order)
//   lam  <- gx_h + g_q[:nx],   dU_h = g_q[nx:],   Lam <- sym(gS_h) + A_h^T Lam A_h
// One workgroup per rollout r, thread (i, j) = (tid >> 4, tid & 15); sequential, fixed-order sums; the lower triangle of the new
// Lam is formed and mirrored.  lam and Lam are updated in place (this workgroup alone touches row r of either).
struct PropAdj {
  const double* shares;              // groups x (NO R) x D, entry e = o * so + r * sm
  const double* sdvar;               // the stage's variance gradient, normalised-target units, per unit of the scaled query:
  int groups, dvo;                   // ... output o, rollout r at [(o * dvo + r) * D + d]
  int coord_of[16];                  // output -> state coordinate
  double ystd2[16];
};

__global__ __launch_bounds__(256) void propagate_adjoint_kernel(PropK k, PropAdj a, int R, int H, int h,
                                                                const double* __restrict__ sjac, const double* __restrict__ lin,
                                                                const double* __restrict__ gx_h, const double* __restrict__ gS_h,
                                                                double* lam, double* Lam, double* dU) {
  __shared__ double A[16][17], L[16][17], T[16][17], J[16][17], GV[16][17], HW[16][17];
  __shared__ double lm[16];
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, r = blockIdx.x;
  const int nx = k.nx, D = k.D, NO = k.NO, nu = D - nx;
  if (i < nx && j < nx) L[i][j] = Lam[((long long)r * nx + i) * nx + j];
  if (tid < nx) lm[tid] = lam[(long long)r * nx + tid];
  if (i < NO && j < D) {
    const long long E = (long long)NO * R, e = i * k.so + r * k.sm;
    const double g = sjac[e * D + j];
    J[i][j] = k.scaled ? g / k.in_scale[j] : g;
    const double dv = a.sdvar[((long long)i * a.dvo + r) * D + j] * a.ystd2[i];
    GV[i][j] = k.scaled ? dv / k.in_scale[j] : dv;
    double s = 0.0;
#pragma unroll 8
    for (int g2 = 0; g2 < a.groups; ++g2) s += a.shares[(g2 * E + e) * D + j];
    HW[i][j] = s;
  }
  __syncthreads();
  if (i < nx && j < nx) {
    const int o = k.model_of[i];
    double v = (i == j ? 1.0 : 0.0) + lin[i * D + j];
    if (o >= 0) v += J[o][j];
    A[i][j] = v;
  }
  if (tid < D) {      // thread d forms g_q[d]
    const int d = tid;
    double s = 0.0;
    for (int c = 0; c < nx; ++c) {
      const int o = k.model_of[c];
      double f = (c == d ? 1.0 : 0.0) + lin[c * D + d];
      if (o >= 0) f += J[o][d];
      s = __builtin_fma(f, lm[c], s);
    }
    for (int o = 0; o < NO; ++o) {
      const int c = a.coord_of[o];
      s = __builtin_fma(L[c][c], GV[o][d], s);
      s = __builtin_fma(2.0, HW[o][d], s);
    }
    if (d < nx) lam[(long long)r * nx + d] = gx_h[(long long)r * nx + d] + s;
    else dU[((long long)r * H + h) * nu + (d - nx)] = s;
  }
  __syncthreads();
  if (i < nx && j < nx) {
    double t = 0.0;
    for (int c = 0; c < nx; ++c) t = __builtin_fma(L[i][c], A[c][j], t);
    T[i][j] = t;
  }
  __syncthreads();
  if (i < nx && j <= i) {
    double s = 0.0;
    for (int c = 0; c < nx; ++c) s = __builtin_fma(A[c][i], T[c][j], s);
    const long long at = (long long)r * nx * nx;
    if (gS_h) s += gS_h[at + i * nx + j];
    Lam[at + i * nx + j] = s;
    Lam[at + j * nx + i] = s;
  }
}

}  // namespace

// ---- the skeleton (gpk_internal.h) ------------------------------------------------------------------------------------------------
HorizonBlock::HorizonBlock(int nx_, int D_, const Horizon& z) : nx(nx_), D(D_), nu(D_ - nx_), R(z.R), H(z.H) {
  n_x = (size_t)R * nx; n_s = n_x * nx; n_q = (size_t)R * D; n_lin = (size_t)nx * D; n_Q = (size_t)nx * nx;
  n_u = nu ? (size_t)z.u_rows * H * nu : 0;
  u_row_stride = (nu && z.u_rows == R) ? (long long)H * nu : 0;
}

void HorizonBlock::head() {
  x = take(n_x); S = take(n_s); q = take(n_q); lin = take(n_lin); Q = take(n_Q); u = take(n_u);
}

void HorizonBlock::outputs(size_t n0, double* h0, size_t n1, double* h1, size_t n2, double* h2) {
  traj = take((size_t)H * n_x);
  sig = take((size_t)H * n_s);
  const size_t n[3] = {n0, n1, n2};
  double* const host[3] = {h0, h1, h2};
  for (int i = 0; i < 3; ++i) {
    n_out[i] = n[i];
    host_out[i] = host[i];
    out[i] = take((size_t)H * n[i]);
  }
}

int gpk_horizon_check(gpk_handle h, const std::string& who, int nx, int D, const Horizon& z) {
  const int nu = D - nx, R = z.R, H = z.H;
  GPK_REQUIRE(h, R >= 1 && R <= GPK_PROP_MAX_R, who + "R must be in [1, 32]");
  GPK_REQUIRE(h, H >= 1 && H <= GPK_PROP_MAX_H, who + "H must be in [1, 256]");
  GPK_REQUIRE(h, z.x0 && z.lin && z.traj && z.Sigma, who + "null pointer");
  GPK_REQUIRE(h, nu == 0 || z.U, who + "null controls");
  GPK_REQUIRE(h, z.x0_rows == 1 || z.x0_rows == R, who + "x0 must have 1 or R rows");
  GPK_REQUIRE(h, nu == 0 || z.u_rows == 1 || z.u_rows == R, who + "U must have 1 or R rows");
  GPK_REQUIRE(h, !z.Sigma0 || z.s_rows == 1 || z.s_rows == R, who + "Sigma0 must have 1 or R rows");
  const size_t n_Q = (size_t)nx * nx, n_u = nu ? (size_t)z.u_rows * H * nu : 0;
  GPK_REQUIRE(h, gpk_finite(z.x0, (size_t)z.x0_rows * nx) && gpk_finite(z.lin, (size_t)nx * D) && (!n_u || gpk_finite(z.U, n_u)) &&
                     (!z.Q || gpk_finite(z.Q, n_Q)),
              who + "x0, U, lin and Q must not contain NaN or infinity");
  GPK_REQUIRE(h, !z.Sigma0 || gpk_finite(z.Sigma0, (size_t)z.s_rows * n_Q), who + "Sigma0 must not contain NaN or infinity");
  return GPK_OK;
}

void gpk_horizon_pack(const HorizonBlock& b, const Horizon& z, bool scaled, const double* in_shift, const double* in_scale, double* hx) {
  const int nx = b.nx, D = b.D, nu = b.nu, R = b.R, H = b.H;
  double* hS = hx + b.n_x;
  double* hq = hS + b.n_s;
  for (int r = 0; r < R; ++r) {
    const double* xr = z.x0 + (z.x0_rows == 1 ? 0 : (size_t)r * nx);
    memcpy(hx + (size_t)r * nx, xr, sizeof(double) * nx);
    if (z.Sigma0) {
      // the lower triangle is the matrix: mirrored here as every later stage is
      const double* s0 = z.Sigma0 + (z.s_rows == 1 ? 0 : (size_t)r * b.n_Q);
      for (int i = 0; i < nx; ++i)
        for (int j = 0; j <= i; ++j) hS[(size_t)r * b.n_Q + i * nx + j] = hS[(size_t)r * b.n_Q + j * nx + i] = s0[i * nx + j];
    }
    for (int d = 0; d < D; ++d) {
      const double raw = d < nx ? xr[d] : z.U[(z.u_rows == 1 ? 0 : (size_t)r * H * nu) + (d - nx)];
      hq[(size_t)r * D + d] = scaled ? (raw - in_shift[d]) / in_scale[d] : raw;
    }
  }
  // (the kernels read the lower triangle of Q alone)
  memcpy(hq + b.n_q, z.lin, sizeof(double) * b.n_lin);
  if (z.Q) memcpy(hq + b.n_q + b.n_lin, z.Q, sizeof(double) * b.n_Q);
  if (b.n_u) memcpy(hq + b.n_q + b.n_lin + b.n_Q, z.U, sizeof(double) * b.n_u);
}

int gpk_horizon_upload(gpk_handle h, const HorizonBlock& b, const Horizon& z, const std::vector<double>& host) {
  memcpy(z.traj, host.data(), sizeof(double) * b.n_x);
  memcpy(z.Sigma, host.data() + b.n_x, sizeof(double) * b.n_s);
  GPK_CHECK_HIP(h, hipMemcpyAsync(b.x, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, h->stream));
  return GPK_OK;
}

StageView gpk_horizon_stage(const HorizonBlock& b, const Horizon& z, int s) {
  const bool last = s + 1 == b.H;
  StageView v{};
  v.lin = b.lin;
  v.Qn = z.Q ? b.Q : nullptr;
  v.u = b.u + (size_t)s * b.nu;
  v.u_next = b.u + (size_t)(last ? s : s + 1) * b.nu;
  v.u_row_stride = b.u_row_stride;
  v.x = b.x;
  v.S = b.S;
  v.qnext = last ? nullptr : b.queries(s + 1);
  v.traj_next = b.traj + (size_t)s * b.n_x;
  v.sig_next = b.sig + (size_t)s * b.n_s;
  for (int i = 0; i < 3; ++i) v.out[i] = b.host_out[i] ? b.out[i] + (size_t)s * b.n_out[i] : nullptr;
  return v;
}

int gpk_horizon_finish(gpk_handle h, const HorizonBlock& b, const Horizon& z, std::initializer_list<HorizonCopy> more) {
  const size_t H = (size_t)b.H;
  GPK_CHECK_HIP(h, hipMemcpyAsync(z.traj + b.n_x, b.traj, sizeof(double) * H * b.n_x, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(z.Sigma + b.n_s, b.sig, sizeof(double) * H * b.n_s, hipMemcpyDeviceToHost, h->stream));
  for (int i = 0; i < 3; ++i)
    if (b.host_out[i])
      GPK_CHECK_HIP(h, hipMemcpyAsync(b.host_out[i], b.out[i], sizeof(double) * H * b.n_out[i], hipMemcpyDeviceToHost, h->stream));
  for (const HorizonCopy& c : more)
    if (c.dst && c.n) GPK_CHECK_HIP(h, hipMemcpyAsync(c.dst, c.src, sizeof(double) * c.n, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  return GPK_OK;
}

namespace {

// The chain's own device buffers: the stage's small-batch results and work area.  jac_step / dvar_step: doubles between the stages'
// Jacobians and variance gradients where the chain keeps them (0: the stage's are reused; dvar null: none are formed).
struct ChainBuffers {
  double *mean, *var, *jac, *dvar, *work;
  size_t jac_step, dvar_step;
  double *shares, *trs, *corr;       // order 2: the trace launch's shares, tr St per (model, rollout), c of every stage
};

// The forward stages of the linear chain and of the gradient chain: the launches of `call` (GPK_SMALL_JACVAR, or GPK_SMALL_GRAD
// with the variance gradient; mean, Jacobian and variance have the same bits) on the stage's queries, at order 2 the trace launch,
// then the advance launch, which GPK_TIMED_PROPAGATE brackets.
int propagate_forward(gpk_handle h, int call, const ServeModels& m, const PropK& k, const Horizon& z, const HorizonBlock& b,
                      const ChainBuffers& c) {
  const int R = z.R, NO = k.NO;
  const bool second = z.order == 2;
  Prop2 p2{};
  if (second) {
    p2.shares = c.shares; p2.trs = c.trs; p2.groups = (int)gpk_small_trace_groups(m.Np); p2.tro = m.B > 1 ? R : 0;
    for (int o = 0; o < NO; ++o) p2.ystd[o] = m.y_std[o];
  }
  for (int s = 0; s < z.H; ++s) {
    double* jac = c.jac + (size_t)s * c.jac_step;
    const ServeOut stage{c.mean, c.var, jac, c.dvar ? c.dvar + (size_t)s * c.dvar_step : nullptr, nullptr};
    GPK_TRY(gpk_small_launch(h, call, m, b.queries(s), R, c.work, stage));
    const StageView v = gpk_horizon_stage(b, z, s);
    if (second) {
      GPK_TRY(gpk_small_trace_launch(h, m, b.q, R, b.S, k.nx, k.in_scale, c.shares, c.trs));
      p2.ocorr = z.corr ? c.corr + (size_t)s * NO * R : nullptr;
      gpk_time_begin(h, GPK_TIMED_PROPAGATE);
      hipLaunchKernelGGL(propagate_advance2_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, v, R, (const double*)c.mean,
                         (const double*)c.var, jac, p2);
    } else {
      gpk_time_begin(h, GPK_TIMED_PROPAGATE);
      hipLaunchKernelGGL(propagate_advance_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, v, R, (const double*)c.mean,
                         (const double*)c.var, jac);
    }
    gpk_time_end(h);
    GPK_LAUNCH_CHECK(h);
  }
  return GPK_OK;
}

int propagate_run_grad(gpk_handle h, const ServeModels& m, const PropK& k, const Horizon& z);

}  // namespace

int gpk_propagate_run(gpk_handle h, const std::string& who, const ServeModels& m, PropK k, const Horizon& z) {
  const int nx = k.nx, D = k.D, nu = D - nx, NO = k.NO, R = z.R, H = z.H;
  GPK_REQUIRE(h, h->batch == 1, who + "not available in batched mode");
  GPK_REQUIRE(h, z.order == 1 || z.order == 2, who + "order must be 1 or 2");
  GPK_REQUIRE(h, D >= 1 && D <= PROP_MAX_D && nx >= 1 && nx <= PROP_MAX_NX && nx <= D, who + "needs 1 <= nx <= D <= 16");
  GPK_REQUIRE(h, m.N >= 1 && gpk_padded(m.N) <= GPK_SMALL_MAX_NP && m.Np == gpk_padded(m.N) && m.ldw >= m.Np,
              who + "needs N <= 16384, Np = gpk_padded(N) and ldw >= Np");
  // the model's host arrays go into the kernels' parameter blocks as they are
  GPK_REQUIRE(h, gpk_finite(m.ls, (size_t)m.B * D) && gpk_finite(m.sf2, m.B) && gpk_finite(m.y_mean, (size_t)m.B * m.P) &&
                     gpk_finite(m.y_std, (size_t)m.B * m.P),
              who + "ls, sf2, y_mean and y_std must not contain NaN or infinity");
  for (int i = 0; i < m.B * D; ++i) GPK_REQUIRE(h, m.ls[i] > 0.0, who + "length-scales must be positive");
  GPK_TRY(gpk_horizon_check(h, who, nx, D, z));
  if (z.grad) {
    const HorizonGrad& g = *z.grad;
    GPK_REQUIRE(h, z.order == 1, who + "the gradient is that of the first-order propagation (order = 1)");
    GPK_REQUIRE(h, g.gx && g.dx0, who + "null seed gx or null result dx0");
    GPK_REQUIRE(h, nu == 0 || g.dU, who + "null result dU");
    GPK_REQUIRE(h, gpk_finite(g.gx, (size_t)(H + 1) * R * nx) && (!g.gS || gpk_finite(g.gS, (size_t)(H + 1) * R * nx * nx)),
                who + "the seeds gx and gS must not contain NaN or infinity");
    return propagate_run_grad(h, m, k, z);
  }
  // order 2: the trace launch's shares (groups x NO R x 2), tr St per (model, rollout), and c of every stage
  const bool second = z.order == 2;
  const unsigned groups = second ? gpk_small_trace_groups(m.Np) : 0;
  GPK_REQUIRE(h, groups <= (unsigned)PROP_MAX_GROUPS, who + "more trace workgroups than the advance launch adds");
  // the device block: the upload's head, the stage's results, the small-batch work area, the horizon's outputs
  const size_t n_sm = (size_t)NO * R, n_sj = n_sm * D;
  HorizonBlock b(nx, D, z);
  ChainBuffers c{};
  GPK_TRY(gpk_horizon_carve(h, b, [&] {
    b.head();
    c.mean = b.take(n_sm);
    c.var = b.take(n_sm);
    c.jac = b.take(n_sj);
    c.work = b.take(gpk_small_work_doubles(GPK_SMALL_JACVAR, m.Np, m.B, R, D, m.P, m.F));
    b.outputs(n_sm, z.mean, n_sm, z.var, n_sj, z.jac);
    c.shares = b.take((size_t)groups * n_sm * 2);
    c.trs = b.take(second ? (size_t)m.B * R : 0);
    c.corr = b.take(second ? (size_t)H * n_sm : 0);
  }));
  std::vector<double> host(b.n_head(), 0.0);
  gpk_horizon_pack(b, z, k.scaled, k.in_shift, k.in_scale, host.data());
  GPK_TRY(gpk_horizon_upload(h, b, z, host));
  GPK_TRY(propagate_forward(h, GPK_SMALL_JACVAR, m, k, z, b, c));
  if (z.corr && !second) memset(z.corr, 0, sizeof(double) * H * n_sm);
  return gpk_horizon_finish(h, b, z, {{second ? z.corr : nullptr, c.corr, (size_t)H * n_sm}});
}

namespace {

// The chain with the backward sweep (z.grad; every argument checked by gpk_propagate_run).  Forward: propagate_forward on the
// three launches of GPK_SMALL_GRAD; the scaled queries, the Jacobians and the variance gradients of every stage stay in the
// device block, Sigma_h in the horizon's own output (Sigma_0: a second copy in the upload).  Backward, per stage: the
// Hessian-vector launch and propagate_adjoint_kernel.  6 H launches, one upload [head | S_0 | lam = gx_H | Lam = sym gS_H | gx |
// sym gS], one synchronisation, the downloads after the last launch.
int propagate_run_grad(gpk_handle h, const ServeModels& m, const PropK& k, const Horizon& z) {
  const HorizonGrad& g = *z.grad;
  const int nx = k.nx, D = k.D, nu = D - nx, NO = k.NO, R = z.R, H = z.H;
  const unsigned groups = gpk_small_trace_groups(m.Np);
  GPK_REQUIRE(h, groups <= (unsigned)PROP_MAX_GROUPS, "propagate: more Hessian-vector workgroups than the adjoint launch adds");
  const size_t n_sm = (size_t)NO * R, n_sj = n_sm * D, n_dv = (size_t)m.B * R * D, n_du = (size_t)R * H * nu;
  HorizonBlock b(nx, D, z);
  const size_t n_x = b.n_x, n_s = b.n_s, n_Q = b.n_Q, n_gx = (size_t)H * n_x, n_gS = g.gS ? (size_t)H * n_s : 0;
  ChainBuffers c{};
  c.jac_step = n_sj;
  c.dvar_step = n_dv;
  double *d_S0, *d_lam, *d_Lam, *d_gx, *d_gS, *d_sh, *d_du;
  GPK_TRY(gpk_horizon_carve(h, b, [&] {
    b.head();
    d_S0 = b.take(n_s); d_lam = b.take(n_x); d_Lam = b.take(n_s); d_gx = b.take(n_gx); d_gS = b.take(n_gS);      // (uploaded)
    c.mean = b.take(n_sm);
    c.var = b.take(n_sm);
    c.work = b.take(gpk_small_work_doubles(GPK_SMALL_GRAD, m.Np, m.B, R, D, m.P, m.F));
    b.outputs(n_sm, z.mean, n_sm, z.var, n_sj, z.jac);
    b.qs = b.take((size_t)(H - 1) * b.n_q);
    c.jac = b.take((size_t)H * n_sj);
    c.dvar = b.take((size_t)H * n_dv);
    d_sh = b.take((size_t)groups * n_sj);
    d_du = b.take(n_du);
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
  GPK_TRY(propagate_forward(h, GPK_SMALL_GRAD, m, k, z, b, c));
  SmallHvp hv{};
  PropAdj pa{};
  hv.Lam = d_Lam; hv.lin = b.lin; hv.nx = nx; hv.so = k.so; hv.sm = k.sm; hv.scaled = k.scaled;
  pa.shares = d_sh; pa.groups = (int)groups; pa.dvo = m.B > 1 ? R : 0;
  for (int d = 0; d < 16; ++d) { hv.model_of[d] = k.model_of[d]; hv.in_scale[d] = k.in_scale[d]; hv.coord_of[d] = pa.coord_of[d] = -1; }
  for (int c2 = 0; c2 < nx; ++c2)
    if (k.model_of[c2] >= 0) hv.coord_of[k.model_of[c2]] = pa.coord_of[k.model_of[c2]] = c2;
  for (int o = 0; o < NO; ++o) pa.ystd2[o] = m.y_std[o] * m.y_std[o];
  for (int s = H - 1; s >= 0; --s) {
    hv.Sg = s == 0 ? d_S0 : b.sig + (size_t)(s - 1) * n_s;
    hv.sjac = c.jac + (size_t)s * n_sj;
    pa.sdvar = c.dvar + (size_t)s * n_dv;
    GPK_TRY(gpk_small_hvp_launch(h, m, b.queries(s), R, hv, d_sh));
    hipLaunchKernelGGL(propagate_adjoint_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, pa, R, H, s, hv.sjac,
                       (const double*)b.lin, (const double*)(d_gx + (size_t)s * n_x),
                       g.gS ? (const double*)(d_gS + (size_t)s * n_s) : nullptr, d_lam, d_Lam, d_du);
    GPK_LAUNCH_CHECK(h);
  }
  return gpk_horizon_finish(h, b, z, {{g.dU, d_du, n_du}, {g.dx0, d_lam, n_x}, {g.dSigma0, d_Lam, n_s}});
}

}  // namespace

// The single-model entries' body: m with B = 1, pointers to the entry's scalars, P the state width.  `who`: the entry's name in
// the messages.
static int propagate_host_any(gpk_handle h, const std::string& who, const HostModels& a, const Horizon& z) {
  if (!h) return GPK_BAD_ARG;
  const int P = a.P, D = a.D;
  GPK_REQUIRE(h, *a.X && *a.alpha && a.ls && a.y_mean && a.y_std && *a.W, who + "null pointer");
  GPK_REQUIRE(h, P >= 1 && P <= GPK_MAX_P && P <= D, who + "the state dimension P must be in [1, 16] and must not exceed D");
  GPK_REQUIRE(h, gpk_finite(a.noise, 1) && gpk_finite(a.kss, 1) && gpk_finite(&a.floor_, 1), who + "kss, floor and noise must be finite");
  PropK k{};
  k.nx = P; k.D = D; k.NO = P;
  k.so = 1; k.sm = P; k.vo = 0; k.vm = 1;
  k.add_noise = a.var_includes_noise != 0;
  for (int d = 0; d < 16; ++d) { k.in_shift[d] = 0.0; k.in_scale[d] = 1.0; k.model_of[d] = d < P ? d : -1; }
  for (int p = 0; p < P; ++p) { k.ystd2[p] = a.y_std[p] * a.y_std[p]; k.noise[p] = *a.noise; }
  const ServeModels m{1, P, 1, a.X, a.alpha, a.N, D, a.ls, a.sf2, a.y_mean, a.y_std, {a.W, nullptr}, a.Np, a.ldw, a.kss, a.floor_, nullptr};
  return gpk_propagate_run(h, who, m, k, z);
}

// The batch entries' body, as propagate_host_any.
static int propagate_host_multi_any(gpk_handle h, const std::string& who, const HostModels& a, const Horizon& z) {
  if (!h) return GPK_BAD_ARG;
  const int B = a.B, D = a.D, nx = a.nx;
  GPK_REQUIRE(h, a.X && a.alpha && a.ls && a.sf2 && a.y_mean && a.y_std && a.W && a.kss && a.coord, who + "null pointer");
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, who + "1..8 models");
  GPK_REQUIRE(h, D >= 1 && D <= PROP_MAX_D && nx >= B && nx <= D, who + "the state dimension nx must be in [B, D], D <= 16");
  GPK_REQUIRE(h, !a.var_includes_noise || a.noise, who + "null noise levels");
  GPK_REQUIRE(h, (a.in_shift == nullptr) == (a.in_scale == nullptr), who + "in_shift and in_scale go together");
  for (int b = 0; b < B; ++b) GPK_REQUIRE(h, a.X[b] && a.alpha[b] && a.W[b], who + "null model pointer");
  PropK k{};
  k.nx = nx; k.D = D; k.NO = B;
  k.so = z.R; k.sm = 1; k.vo = z.R; k.vm = 1;
  k.add_noise = a.var_includes_noise != 0;
  for (int d = 0; d < 16; ++d) { k.in_shift[d] = 0.0; k.in_scale[d] = 1.0; k.model_of[d] = -1; }
  for (int b = 0; b < B; ++b) {
    GPK_REQUIRE(h, a.coord[b] >= 0 && a.coord[b] < nx, who + "coord must be in [0, nx)");
    GPK_REQUIRE(h, k.model_of[a.coord[b]] < 0, who + "coord must be distinct");
    k.model_of[a.coord[b]] = b;
    k.ystd2[b] = a.y_std[b] * a.y_std[b];
    k.noise[b] = a.var_includes_noise ? a.noise[b] : 0.0;
  }
  GPK_REQUIRE(h, gpk_finite(a.kss, B) && gpk_finite(k.noise, B) && gpk_finite(&a.floor_, 1), who + "kss, floor and noise must be finite");
  if (a.in_shift) {
    GPK_REQUIRE(h, gpk_finite(a.in_shift, D) && gpk_finite(a.in_scale, D), who + "the input scaler must not contain NaN or infinity");
    for (int d = 0; d < D; ++d) {
      GPK_REQUIRE(h, a.in_scale[d] != 0.0, who + "in_scale must be non-zero");
      k.in_shift[d] = a.in_shift[d];
      k.in_scale[d] = a.in_scale[d];
    }
    k.scaled = 1;
  }
  const ServeModels m{B, 1, 1, a.X, a.alpha, a.N, D, a.ls, a.sf2, a.y_mean, a.y_std, {a.W, nullptr}, a.Np, a.ldw, a.kss, a.floor_, nullptr};
  return gpk_propagate_run(h, who, m, k, z);
}

extern "C" int gpk_propagate_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                  double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np, int64_t ldw,
                                  double kss, double floor_, int var_includes_noise, double noise, const double* x0, int x0_rows,
                                  const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q,
                                  int R, int H, double* traj, double* Sigma, double* mean, double* var, double* jac) {
  const HostModels a{1, P, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, &W, Np, ldw, &kss, floor_, var_includes_noise, &noise, P};
  return propagate_host_any(h, "propagate_host: ", a, Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac});
}

extern "C" int gpk_propagate2_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                   double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np, int64_t ldw,
                                   double kss, double floor_, int var_includes_noise, double noise, const double* x0, int x0_rows,
                                   const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q,
                                   int R, int H, double* traj, double* Sigma, double* mean, double* var, double* jac, int order,
                                   double* corr) {
  const HostModels a{1, P, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, &W, Np, ldw, &kss, floor_, var_includes_noise, &noise, P};
  return propagate_host_any(h, "propagate2_host: ", a,
                            Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, order, corr});
}

extern "C" int gpk_propagate_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                        const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                        const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                        int var_includes_noise, const double* noise, int nx, const int* coord,
                                        const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                        const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                        const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                        double* jac) {
  const HostModels a{B, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_, var_includes_noise, noise, nx, coord,
                     in_shift, in_scale};
  return propagate_host_multi_any(h, "propagate_host_multi: ", a,
                                  Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac});
}

extern "C" int gpk_propagate2_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                         const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                         const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                         int var_includes_noise, const double* noise, int nx, const int* coord,
                                         const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                         const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                         const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                         double* jac, int order, double* corr) {
  const HostModels a{B, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_, var_includes_noise, noise, nx, coord,
                     in_shift, in_scale};
  return propagate_host_multi_any(h, "propagate2_host_multi: ", a,
                                  Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, order, corr});
}

// ... with the gradient of a horizon cost (order 1): the seeds gx, gS and the results dU, dx0, dSigma0 as HorizonGrad describes them
extern "C" int gpk_propagate_grad_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                       double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np,
                                       int64_t ldw, double kss, double floor_, int var_includes_noise, double noise, const double* x0,
                                       int x0_rows, const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                       const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                       double* jac, const double* gx, const double* gS, double* dU, double* dx0, double* dSigma0) {
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  const HostModels a{1, P, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, &W, Np, ldw, &kss, floor_, var_includes_noise, &noise, P};
  return propagate_host_any(h, "propagate_grad_host: ", a,
                            Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, 1, nullptr, &g});
}

extern "C" int gpk_propagate_grad_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                             const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                             const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                             int var_includes_noise, const double* noise, int nx, const int* coord,
                                             const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                             const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                             const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                             double* jac, const double* gx, const double* gS, double* dU, double* dx0,
                                             double* dSigma0) {
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  const HostModels a{B, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_, var_includes_noise, noise, nx, coord,
                     in_shift, in_scale};
  return propagate_host_multi_any(h, "propagate_grad_host_multi: ", a,
                                  Horizon{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, 1, nullptr, &g});
}
