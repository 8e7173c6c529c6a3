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
// those copies and may wait on them by itself; nothing waits between the stages.  gpk_propagate_run is the chain for every entry:
// the exact models' below, the sparse models' in gpk_sparse.hip (two inverse factors per model: the stage's variance arrives final
// and in another layout, which PropK's strides describe).
//
// The gradient of a horizon cost (Horizon::grad; order 1): the same forward stages on the three launches of GPK_SMALL_GRAD - the
// variance gradient comes with them, mean, Jacobian and variance keep their bits - with every stage's queries, Jacobians and
// variance gradients kept in the device block, then per stage, backwards, the Hessian-vector launch (small_hvp_kernel,
// gpk_small.hip) and propagate_adjoint_kernel below: 6 H launches, the seeds in the one upload, still ONE synchronisation
// (propagate_run_grad).
#include "gpk_internal.h"

namespace {

constexpr int PROP_MAX_R = GPK_PROP_MAX_R, PROP_MAX_H = GPK_PROP_MAX_H, PROP_MAX_NX = GPK_PROP_MAX_NX, PROP_MAX_D = GPK_PROP_MAX_D;
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
__device__ __forceinline__ void propagate_advance_body(PropK k, int R, const double* __restrict__ smean,
                                                       const double* __restrict__ svar, const double* __restrict__ sjac,
                                                       const double* __restrict__ lin, const double* __restrict__ Qn,
                                                       const double* __restrict__ u, const double* __restrict__ u_next,
                                                       long long u_row_stride, double* x, double* S, double* qnext,
                                                       double* traj_next, double* sig_next, double* omean, double* ovar,
                                                       double* ojac, const Prop2* p2) {
  __shared__ double A[16][17], Sg[16][17], T[16][17], J[16][17];
  __shared__ double q[16], mu[16], vv[16], xn[16];
  [[maybe_unused]] double (*cc)[16] = nullptr;
  if constexpr (SECOND) {
    __shared__ double cc_s[16];
    cc = &cc_s;
  }
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, r = blockIdx.x;
  const int nx = k.nx, D = k.D, NO = k.NO;
  if (tid < D) q[tid] = tid < nx ? x[(long long)r * nx + tid] : u[r * u_row_stride + (tid - nx)];
  if (i < nx && j < nx) Sg[i][j] = S[((long long)r * nx + i) * nx + j];
  if (tid < NO) {
    const double v = svar[tid * k.vo + r * k.vm];
    mu[tid] = smean[tid * k.so + r * k.sm];
    vv[tid] = (k.add_noise ? v + k.noise[tid] : v) * k.ystd2[tid];
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
    double a = (i == j ? 1.0 : 0.0) + lin[i * D + j];
    if (o >= 0) a += J[o][j];
    A[i][j] = a;
  }
  if (tid < nx) {
    const int o = k.model_of[tid];
    double a = 0.0;
    for (int d = 0; d < D; ++d) a = __builtin_fma(lin[tid * D + d], q[d], a);
    double v = q[tid] + a;
    if (o >= 0) v += mu[o];
    xn[tid] = v;
  }
  __syncthreads();
  if (i < nx && j < nx) {
    double t = 0.0;
    for (int c = 0; c < nx; ++c) t = __builtin_fma(A[i][c], Sg[c][j], t);
    T[i][j] = t;
  }
  __syncthreads();
  if (i < nx && j <= i) {
    double s = 0.0;
    for (int c = 0; c < nx; ++c) s = __builtin_fma(T[i][c], A[j][c], s);
    const int o = k.model_of[i];
    if (i == j && o >= 0) s += vv[o];
    if (Qn) s += Qn[i * nx + j];
    const long long at = (long long)r * nx * nx;
    S[at + i * nx + j] = s;
    S[at + j * nx + i] = s;
    sig_next[at + i * nx + j] = s;
    sig_next[at + j * nx + i] = s;
  }
  if constexpr (SECOND) {
    if (tid < nx) {
      const int o = k.model_of[tid];
      if (o >= 0) xn[tid] += (*cc)[o];
    }
    if (p2->ocorr && tid < NO) p2->ocorr[(long long)r * NO + tid] = (*cc)[tid];
  }
  if (tid < nx) {
    x[(long long)r * nx + tid] = xn[tid];
    traj_next[(long long)r * nx + tid] = xn[tid];
  }
  if (qnext && tid < D) {
    const double raw = tid < nx ? xn[tid] : u_next[r * u_row_stride + (tid - nx)];
    qnext[(long long)r * D + tid] = k.scaled ? (raw - k.in_shift[tid]) / k.in_scale[tid] : raw;
  }
  if (tid < NO) {
    if (omean) omean[(long long)r * NO + tid] = mu[tid];
    if (ovar) ovar[(long long)r * NO + tid] = vv[tid];
  }
  if (ojac && i < NO && j < D) ojac[((long long)r * NO + i) * D + j] = J[i][j];
}

__global__ __launch_bounds__(256) void propagate_advance_kernel(PropK k, int R, const double* __restrict__ smean,
                                                                const double* __restrict__ svar, const double* __restrict__ sjac,
                                                                const double* __restrict__ lin, const double* __restrict__ Qn,
                                                                const double* __restrict__ u, const double* __restrict__ u_next,
                                                                long long u_row_stride, double* x, double* S, double* qnext,
                                                                double* traj_next, double* sig_next, double* omean, double* ovar,
                                                                double* ojac) {
  propagate_advance_body<false>(k, R, smean, svar, sjac, lin, Qn, u, u_next, u_row_stride, x, S, qnext, traj_next, sig_next, omean, ovar,
                                ojac, nullptr);
}
__global__ __launch_bounds__(256) void propagate_advance2_kernel(PropK k, int R, const double* __restrict__ smean,
                                                                 const double* __restrict__ svar, const double* __restrict__ sjac,
                                                                 const double* __restrict__ lin, const double* __restrict__ Qn,
                                                                 const double* __restrict__ u, const double* __restrict__ u_next,
                                                                 long long u_row_stride, double* x, double* S, double* qnext,
                                                                 double* traj_next, double* sig_next, double* omean, double* ovar,
                                                                 double* ojac, Prop2 p2) {
  propagate_advance_body<true>(k, R, smean, svar, sjac, lin, Qn, u, u_next, u_row_stride, x, S, qnext, traj_next, sig_next, omean, ovar,
                               ojac, &p2);
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

bool prop_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(p[i] - p[i] == 0.0)) return false;
  return true;
}

// The head of the one upload, [x | S | q | lin | Q | U] (zero-initialised by the caller): the start rows, Sigma0 mirrored from its
// lower triangle, the first stage's scaled queries and the horizon's constants as they come from the host.
void prop_pack(const PropK& k, const Horizon& z, double* hx) {
  const int nx = k.nx, D = k.D, nu = D - nx, R = z.R, H = z.H;
  const size_t n_x = (size_t)R * nx, n_s = n_x * nx, n_q = (size_t)R * D, n_lin = (size_t)nx * D, n_Q = (size_t)nx * nx;
  const size_t n_u = nu ? (size_t)z.u_rows * H * nu : 0;
  double* hS = hx + n_x;
  double* hq = hS + n_s;
  for (int r = 0; r < R; ++r) {
    const double* xr = z.x0 + (z.x0_rows == 1 ? 0 : (size_t)r * nx);
    memcpy(hx + (size_t)r * nx, xr, sizeof(double) * nx);
    if (z.Sigma0) {
      // the lower triangle is the matrix: mirrored here as every later stage is
      const double* s0 = z.Sigma0 + (z.s_rows == 1 ? 0 : (size_t)r * n_Q);
      for (int i = 0; i < nx; ++i)
        for (int j = 0; j <= i; ++j) hS[(size_t)r * n_Q + i * nx + j] = hS[(size_t)r * n_Q + j * nx + i] = s0[i * nx + j];
    }
    for (int d = 0; d < D; ++d) {
      const double raw = d < nx ? xr[d] : z.U[(z.u_rows == 1 ? 0 : (size_t)r * H * nu) + (d - nx)];
      hq[(size_t)r * D + d] = k.scaled ? (raw - k.in_shift[d]) / k.in_scale[d] : raw;
    }
  }
  memcpy(hq + n_q, z.lin, sizeof(double) * n_lin);
  if (z.Q) memcpy(hq + n_q + n_lin, z.Q, sizeof(double) * n_Q);
  if (n_u) memcpy(hq + n_q + n_lin + n_Q, z.U, sizeof(double) * n_u);
}

int propagate_run_grad(gpk_handle h, const ServeModels& m, const PropK& k, const Horizon& z);

}  // namespace

int gpk_propagate_run(gpk_handle h, const std::string& who, const ServeModels& m, PropK k, const Horizon& z) {
  const int nx = k.nx, D = k.D, nu = D - nx, NO = k.NO, R = z.R, H = z.H;
  GPK_REQUIRE(h, h->batch == 1, who + "not available in batched mode");
  GPK_REQUIRE(h, z.order == 1 || z.order == 2, who + "order must be 1 or 2");
  GPK_REQUIRE(h, R >= 1 && R <= PROP_MAX_R, who + "R must be in [1, 32]");
  GPK_REQUIRE(h, H >= 1 && H <= PROP_MAX_H, who + "H must be in [1, 256]");
  GPK_REQUIRE(h, D >= 1 && D <= PROP_MAX_D && nx >= 1 && nx <= PROP_MAX_NX && nx <= D, who + "needs 1 <= nx <= D <= 16");
  GPK_REQUIRE(h, m.N >= 1 && gpk_padded(m.N) <= GPK_SMALL_MAX_NP && m.Np == gpk_padded(m.N) && m.ldw >= m.Np,
              who + "needs N <= 16384, Np = gpk_padded(N) and ldw >= Np");
  // the model's host arrays go into the kernels' parameter blocks as they are
  GPK_REQUIRE(h, prop_finite(m.ls, (size_t)m.B * D) && prop_finite(m.sf2, m.B) && prop_finite(m.y_mean, (size_t)m.B * m.P) &&
                     prop_finite(m.y_std, (size_t)m.B * m.P),
              who + "ls, sf2, y_mean and y_std must not contain NaN or infinity");
  for (int i = 0; i < m.B * D; ++i) GPK_REQUIRE(h, m.ls[i] > 0.0, who + "length-scales must be positive");
  GPK_REQUIRE(h, z.x0 && z.lin && z.traj && z.Sigma, who + "null pointer");
  GPK_REQUIRE(h, nu == 0 || z.U, who + "null controls");
  GPK_REQUIRE(h, z.x0_rows == 1 || z.x0_rows == R, who + "x0 must have 1 or R rows");
  GPK_REQUIRE(h, nu == 0 || z.u_rows == 1 || z.u_rows == R, who + "U must have 1 or R rows");
  GPK_REQUIRE(h, !z.Sigma0 || z.s_rows == 1 || z.s_rows == R, who + "Sigma0 must have 1 or R rows");
  const size_t n_x = (size_t)R * nx, n_s = n_x * nx, n_q = (size_t)R * D, n_lin = (size_t)nx * D, n_Q = (size_t)nx * nx;
  const int u_rows = nu ? z.u_rows : 0;
  const size_t n_u = (size_t)u_rows * H * nu;
  GPK_REQUIRE(h, prop_finite(z.x0, (size_t)z.x0_rows * nx) && prop_finite(z.lin, n_lin) && (!n_u || prop_finite(z.U, n_u)) &&
                     (!z.Sigma0 || prop_finite(z.Sigma0, (size_t)z.s_rows * n_Q)) && (!z.Q || prop_finite(z.Q, n_Q)),
              who + "x0, U, lin, Sigma0 and Q must not contain NaN or infinity");
  if (z.grad) {
    const HorizonGrad& g = *z.grad;
    GPK_REQUIRE(h, z.order == 1, who + "the gradient is that of the first-order propagation (order = 1)");
    GPK_REQUIRE(h, g.gx && g.dx0, who + "null seed gx or null result dx0");
    GPK_REQUIRE(h, nu == 0 || g.dU, who + "null result dU");
    GPK_REQUIRE(h, prop_finite(g.gx, (size_t)(H + 1) * n_x) && (!g.gS || prop_finite(g.gS, (size_t)(H + 1) * n_s)),
                who + "the seeds gx and gS must not contain NaN or infinity");
    return propagate_run_grad(h, m, k, z);
  }
  // the device block: [x | S | q | lin | Q | U] as they come from the host, the stage's results, the small-batch work area, the
  // horizon's outputs from slot 1 on (slot 0 of traj and Sigma is the caller's own start)
  const size_t n_up = n_x + n_s + n_q + n_lin + n_Q + n_u;
  const size_t n_sm = (size_t)NO * R, n_sj = n_sm * D;
  const size_t n_work = gpk_small_work_doubles(GPK_SMALL_JACVAR, m.Np, m.B, R, D, m.P, m.F);
  const size_t n_traj = (size_t)H * n_x, n_sig = (size_t)H * n_s, n_om = (size_t)H * n_sm, n_oj = (size_t)H * n_sj;
  // order 2: the trace launch's shares (groups x NO R x 2), tr St per (model, rollout), and c of every stage
  const bool second = z.order == 2;
  const unsigned groups = second ? gpk_small_trace_groups(m.Np) : 0;
  GPK_REQUIRE(h, groups <= (unsigned)PROP_MAX_GROUPS, who + "more trace workgroups than the advance launch adds");
  const size_t n_sh = (size_t)groups * n_sm * 2, n_tr = second ? (size_t)m.B * R : 0, n_oc = second ? n_om : 0;
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, (n_up + 2 * n_sm + n_sj + n_work + n_traj + n_sig + 2 * n_om + n_oj + n_sh + n_tr + n_oc) * sizeof(double), &ws));
  double* d_x = (double*)ws;
  double* d_S = d_x + n_x;
  double* d_q = d_S + n_s;
  double* d_lin = d_q + n_q;
  double* d_Q = d_lin + n_lin;
  double* d_u = d_Q + n_Q;
  double* s_mean = d_u + n_u;
  double* s_var = s_mean + n_sm;
  double* s_jac = s_var + n_sm;
  double* work = s_jac + n_sj;
  double* d_traj = work + n_work;
  double* d_sig = d_traj + n_traj;
  double* d_om = d_sig + n_sig;
  double* d_ov = d_om + n_om;
  double* d_oj = d_ov + n_om;
  double* d_sh = d_oj + n_oj;
  double* d_tr = d_sh + n_sh;
  double* d_oc = d_tr + n_tr;
  std::vector<double> host(n_up, 0.0);
  prop_pack(k, z, host.data());
  memcpy(z.traj, host.data(), sizeof(double) * n_x);
  memcpy(z.Sigma, host.data() + n_x, sizeof(double) * n_s);
  GPK_CHECK_HIP(h, hipMemcpyAsync(d_x, host.data(), sizeof(double) * n_up, hipMemcpyHostToDevice, h->stream));
  const ServeOut stage{s_mean, s_var, s_jac, nullptr, nullptr};
  const long long u_row_stride = (nu && z.u_rows == R) ? (long long)H * nu : 0;
  Prop2 p2{};
  if (second) {
    p2.shares = d_sh; p2.trs = d_tr; p2.groups = (int)groups; p2.tro = m.B > 1 ? R : 0;
    for (int o = 0; o < NO; ++o) p2.ystd[o] = m.y_std[o];
  }
  for (int s = 0; s < H; ++s) {
    GPK_TRY(gpk_small_launch(h, GPK_SMALL_JACVAR, m, d_q, R, work, stage));
    const bool last = s + 1 == H;
    if (second) {
      GPK_TRY(gpk_small_trace_launch(h, m, d_q, R, d_S, nx, k.in_scale, d_sh, d_tr));
      p2.ocorr = z.corr ? d_oc + (size_t)s * n_sm : nullptr;
      gpk_time_begin(h, GPK_TIMED_PROPAGATE);
      hipLaunchKernelGGL(propagate_advance2_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, R, (const double*)s_mean,
                         (const double*)s_var, (const double*)s_jac, (const double*)d_lin, z.Q ? (const double*)d_Q : nullptr,
                         (const double*)(d_u + (size_t)s * nu), (const double*)(d_u + (size_t)(last ? s : s + 1) * nu), u_row_stride,
                         d_x, d_S, last ? nullptr : d_q, d_traj + (size_t)s * n_x, d_sig + (size_t)s * n_s,
                         z.mean ? d_om + (size_t)s * n_sm : nullptr, z.var ? d_ov + (size_t)s * n_sm : nullptr,
                         z.jac ? d_oj + (size_t)s * n_sj : nullptr, p2);
      gpk_time_end(h);
      GPK_LAUNCH_CHECK(h);
      continue;
    }
    gpk_time_begin(h, GPK_TIMED_PROPAGATE);
    hipLaunchKernelGGL(propagate_advance_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, R, (const double*)s_mean,
                       (const double*)s_var, (const double*)s_jac, (const double*)d_lin, z.Q ? (const double*)d_Q : nullptr,
                       (const double*)(d_u + (size_t)s * nu), (const double*)(d_u + (size_t)(last ? s : s + 1) * nu), u_row_stride,
                       d_x, d_S, last ? nullptr : d_q, d_traj + (size_t)s * n_x, d_sig + (size_t)s * n_s,
                       z.mean ? d_om + (size_t)s * n_sm : nullptr, z.var ? d_ov + (size_t)s * n_sm : nullptr,
                       z.jac ? d_oj + (size_t)s * n_sj : nullptr);
    gpk_time_end(h);
    GPK_LAUNCH_CHECK(h);
  }
  GPK_CHECK_HIP(h, hipMemcpyAsync(z.traj + n_x, d_traj, sizeof(double) * n_traj, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(z.Sigma + n_s, d_sig, sizeof(double) * n_sig, hipMemcpyDeviceToHost, h->stream));
  if (z.mean) GPK_CHECK_HIP(h, hipMemcpyAsync(z.mean, d_om, sizeof(double) * n_om, hipMemcpyDeviceToHost, h->stream));
  if (z.var) GPK_CHECK_HIP(h, hipMemcpyAsync(z.var, d_ov, sizeof(double) * n_om, hipMemcpyDeviceToHost, h->stream));
  if (z.jac) GPK_CHECK_HIP(h, hipMemcpyAsync(z.jac, d_oj, sizeof(double) * n_oj, hipMemcpyDeviceToHost, h->stream));
  if (z.corr && second) GPK_CHECK_HIP(h, hipMemcpyAsync(z.corr, d_oc, sizeof(double) * n_om, hipMemcpyDeviceToHost, h->stream));
  if (z.corr && !second) memset(z.corr, 0, sizeof(double) * n_om);
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  return GPK_OK;
}

namespace {

// The chain with the backward sweep (z.grad; every argument checked by gpk_propagate_run).  Forward, per stage: the three launches
// of GPK_SMALL_GRAD (mean, Jacobian, variance - the bits of the chain's GPK_SMALL_JACVAR - and the variance gradient) and the
// unchanged advance kernel; the scaled queries, the Jacobians and the variance gradients of every stage stay in the device block,
// Sigma_h in the horizon's own output (Sigma_0: a second copy in the upload).  Backward, per stage: the Hessian-vector launch
// and propagate_adjoint_kernel.  6 H launches, one upload [x | S | q | lin | Q | U | S_0 | lam = gx_H | Lam = sym gS_H | gx | sym gS],
// one synchronisation, the downloads after the last launch.
int propagate_run_grad(gpk_handle h, const ServeModels& m, const PropK& k, const Horizon& z) {
  const HorizonGrad& g = *z.grad;
  const int nx = k.nx, D = k.D, nu = D - nx, NO = k.NO, R = z.R, H = z.H;
  const size_t n_x = (size_t)R * nx, n_s = n_x * nx, n_q = (size_t)R * D, n_lin = (size_t)nx * D, n_Q = (size_t)nx * nx;
  const size_t n_u = nu ? (size_t)z.u_rows * H * nu : 0;
  const size_t n_head = n_x + n_s + n_q + n_lin + n_Q + n_u;
  const size_t n_gx = (size_t)H * n_x, n_gS = g.gS ? (size_t)H * n_s : 0;
  const size_t n_up = n_head + n_s + n_x + n_s + n_gx + n_gS;
  const size_t n_sm = (size_t)NO * R, n_sj = n_sm * D, n_dv = (size_t)m.B * R * D;
  const size_t n_work = gpk_small_work_doubles(GPK_SMALL_GRAD, m.Np, m.B, R, D, m.P, m.F);
  const size_t n_traj = (size_t)H * n_x, n_sig = (size_t)H * n_s, n_om = (size_t)H * n_sm, n_oj = (size_t)H * n_sj;
  const unsigned groups = gpk_small_trace_groups(m.Np);
  GPK_REQUIRE(h, groups <= (unsigned)PROP_MAX_GROUPS, "propagate: more Hessian-vector workgroups than the adjoint launch adds");
  const size_t n_sh = (size_t)groups * n_sj, n_du = (size_t)R * H * nu;
  void* ws = nullptr;
  GPK_TRY(gpk_scratch(h, (n_up + 2 * n_sm + n_work + n_traj + n_sig + 2 * n_om + n_oj + (size_t)(H - 1) * n_q + (size_t)H * n_sj +
                          (size_t)H * n_dv + n_sh + n_du) * sizeof(double), &ws));
  double* d_x = (double*)ws;
  double* d_S = d_x + n_x;
  double* d_q = d_S + n_s;
  double* d_lin = d_q + n_q;
  double* d_Q = d_lin + n_lin;
  double* d_u = d_Q + n_Q;
  double* d_S0 = d_u + n_u;
  double* d_lam = d_S0 + n_s;
  double* d_Lam = d_lam + n_x;
  double* d_gx = d_Lam + n_s;
  double* d_gS = d_gx + n_gx;
  double* s_mean = d_gS + n_gS;
  double* s_var = s_mean + n_sm;
  double* work = s_var + n_sm;
  double* d_traj = work + n_work;
  double* d_sig = d_traj + n_traj;
  double* d_om = d_sig + n_sig;
  double* d_ov = d_om + n_om;
  double* d_oj = d_ov + n_om;
  double* d_qs = d_oj + n_oj;            // the scaled queries of stages 1 .. H - 1 (stage 0: d_q)
  double* d_js = d_qs + (size_t)(H - 1) * n_q;
  double* d_dv = d_js + (size_t)H * n_sj;
  double* d_sh = d_dv + (size_t)H * n_dv;
  double* d_du = d_sh + n_sh;
  std::vector<double> host(n_up, 0.0);
  prop_pack(k, z, host.data());
  double* hS0 = host.data() + n_head;
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
  memcpy(z.traj, host.data(), sizeof(double) * n_x);
  memcpy(z.Sigma, host.data() + n_x, sizeof(double) * n_s);
  GPK_CHECK_HIP(h, hipMemcpyAsync(d_x, host.data(), sizeof(double) * n_up, hipMemcpyHostToDevice, h->stream));
  const long long u_row_stride = (nu && z.u_rows == R) ? (long long)H * nu : 0;
  auto queries = [&](int s) { return s == 0 ? d_q : d_qs + (size_t)(s - 1) * n_q; };
  for (int s = 0; s < H; ++s) {
    double* s_jac = d_js + (size_t)s * n_sj;
    const ServeOut stage{s_mean, s_var, s_jac, d_dv + (size_t)s * n_dv, nullptr};
    GPK_TRY(gpk_small_launch(h, GPK_SMALL_GRAD, m, queries(s), R, work, stage));
    const bool last = s + 1 == H;
    gpk_time_begin(h, GPK_TIMED_PROPAGATE);
    hipLaunchKernelGGL(propagate_advance_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, R, (const double*)s_mean,
                       (const double*)s_var, (const double*)s_jac, (const double*)d_lin, z.Q ? (const double*)d_Q : nullptr,
                       (const double*)(d_u + (size_t)s * nu), (const double*)(d_u + (size_t)(last ? s : s + 1) * nu), u_row_stride,
                       d_x, d_S, last ? nullptr : queries(s + 1), d_traj + (size_t)s * n_x, d_sig + (size_t)s * n_s,
                       z.mean ? d_om + (size_t)s * n_sm : nullptr, z.var ? d_ov + (size_t)s * n_sm : nullptr,
                       z.jac ? d_oj + (size_t)s * n_sj : nullptr);
    gpk_time_end(h);
    GPK_LAUNCH_CHECK(h);
  }
  SmallHvp hv{};
  PropAdj pa{};
  hv.Lam = d_Lam; hv.lin = d_lin; hv.nx = nx; hv.so = k.so; hv.sm = k.sm; hv.scaled = k.scaled;
  pa.shares = d_sh; pa.groups = (int)groups; pa.dvo = m.B > 1 ? R : 0;
  for (int d = 0; d < 16; ++d) { hv.model_of[d] = k.model_of[d]; hv.in_scale[d] = k.in_scale[d]; hv.coord_of[d] = pa.coord_of[d] = -1; }
  for (int c = 0; c < nx; ++c)
    if (k.model_of[c] >= 0) hv.coord_of[k.model_of[c]] = pa.coord_of[k.model_of[c]] = c;
  for (int o = 0; o < NO; ++o) pa.ystd2[o] = m.y_std[o] * m.y_std[o];
  for (int s = H - 1; s >= 0; --s) {
    hv.Sg = s == 0 ? d_S0 : d_sig + (size_t)(s - 1) * n_s;
    hv.sjac = d_js + (size_t)s * n_sj;
    pa.sdvar = d_dv + (size_t)s * n_dv;
    GPK_TRY(gpk_small_hvp_launch(h, m, queries(s), R, hv, d_sh));
    hipLaunchKernelGGL(propagate_adjoint_kernel, dim3((unsigned)R), dim3(256), 0, h->stream, k, pa, R, H, s, hv.sjac,
                       (const double*)d_lin, (const double*)(d_gx + (size_t)s * n_x),
                       g.gS ? (const double*)(d_gS + (size_t)s * n_s) : nullptr, d_lam, d_Lam, d_du);
    GPK_LAUNCH_CHECK(h);
  }
  GPK_CHECK_HIP(h, hipMemcpyAsync(z.traj + n_x, d_traj, sizeof(double) * n_traj, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(z.Sigma + n_s, d_sig, sizeof(double) * n_sig, hipMemcpyDeviceToHost, h->stream));
  if (z.mean) GPK_CHECK_HIP(h, hipMemcpyAsync(z.mean, d_om, sizeof(double) * n_om, hipMemcpyDeviceToHost, h->stream));
  if (z.var) GPK_CHECK_HIP(h, hipMemcpyAsync(z.var, d_ov, sizeof(double) * n_om, hipMemcpyDeviceToHost, h->stream));
  if (z.jac) GPK_CHECK_HIP(h, hipMemcpyAsync(z.jac, d_oj, sizeof(double) * n_oj, hipMemcpyDeviceToHost, h->stream));
  if (n_du) GPK_CHECK_HIP(h, hipMemcpyAsync(g.dU, d_du, sizeof(double) * n_du, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipMemcpyAsync(g.dx0, d_lam, sizeof(double) * n_x, hipMemcpyDeviceToHost, h->stream));
  if (g.dSigma0) GPK_CHECK_HIP(h, hipMemcpyAsync(g.dSigma0, d_Lam, sizeof(double) * n_s, hipMemcpyDeviceToHost, h->stream));
  GPK_CHECK_HIP(h, hipStreamSynchronize(h->stream));
  return GPK_OK;
}

}  // namespace

// The single-model entries' body.  `who`: the entry's name in the messages; order and corr as in Horizon.
static int propagate_host_any(gpk_handle h, const std::string& who, const double* X, const double* alpha, int64_t N, int D, int P,
                              const double* ls, double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np,
                              int64_t ldw, double kss, double floor_, int var_includes_noise, double noise, const double* x0,
                              int x0_rows, const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                              const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var, double* jac,
                              int order, double* corr, const HorizonGrad* grad = nullptr) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && ls && y_mean && y_std && W, who + "null pointer");
  GPK_REQUIRE(h, P >= 1 && P <= GPK_MAX_P && P <= D, who + "the state dimension P must be in [1, 16] and must not exceed D");
  GPK_REQUIRE(h, prop_finite(&noise, 1) && prop_finite(&kss, 1) && prop_finite(&floor_, 1), who + "kss, floor and noise must be finite");
  PropK k{};
  k.nx = P; k.D = D; k.NO = P;
  k.so = 1; k.sm = P; k.vo = 0; k.vm = 1;
  k.add_noise = var_includes_noise != 0;
  for (int d = 0; d < 16; ++d) { k.in_shift[d] = 0.0; k.in_scale[d] = 1.0; k.model_of[d] = d < P ? d : -1; }
  for (int p = 0; p < P; ++p) { k.ystd2[p] = y_std[p] * y_std[p]; k.noise[p] = noise; }
  const ServeModels m{1, P, 1, &X, &alpha, N, D, ls, &sf2, y_mean, y_std, {&W, nullptr}, Np, ldw, &kss, floor_, nullptr};
  const Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, order, corr, grad};
  return gpk_propagate_run(h, who, m, k, z);
}

extern "C" int gpk_propagate_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                  double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np, int64_t ldw,
                                  double kss, double floor_, int var_includes_noise, double noise, const double* x0, int x0_rows,
                                  const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q,
                                  int R, int H, double* traj, double* Sigma, double* mean, double* var, double* jac) {
  return propagate_host_any(h, "propagate_host: ", X, alpha, N, D, P, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_, var_includes_noise,
                            noise, x0, x0_rows, U, u_rows, lin, Sigma0, s_rows, Q, R, H, traj, Sigma, mean, var, jac, 1, nullptr);
}

extern "C" int gpk_propagate2_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                   double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np, int64_t ldw,
                                   double kss, double floor_, int var_includes_noise, double noise, const double* x0, int x0_rows,
                                   const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows, const double* Q,
                                   int R, int H, double* traj, double* Sigma, double* mean, double* var, double* jac, int order,
                                   double* corr) {
  return propagate_host_any(h, "propagate2_host: ", X, alpha, N, D, P, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_,
                            var_includes_noise, noise, x0, x0_rows, U, u_rows, lin, Sigma0, s_rows, Q, R, H, traj, Sigma, mean, var, jac,
                            order, corr);
}

// The batch entries' body, as propagate_host_any.
static int propagate_host_multi_any(gpk_handle h, const std::string& who, int B, const double* const* X, const double* const* alpha,
                                    int64_t N, int D, const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                    const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                    int var_includes_noise, const double* noise, int nx, const int* coord, const double* in_shift,
                                    const double* in_scale, const double* x0, int x0_rows, const double* U, int u_rows,
                                    const double* lin, const double* Sigma0, int s_rows, const double* Q, int R, int H, double* traj,
                                    double* Sigma, double* mean, double* var, double* jac, int order, double* corr,
                                    const HorizonGrad* grad = nullptr) {
  if (!h) return GPK_BAD_ARG;
  GPK_REQUIRE(h, X && alpha && ls && sf2 && y_mean && y_std && W && kss && coord, who + "null pointer");
  GPK_REQUIRE(h, B >= 1 && B <= GPK_SMALL_MAX_MODELS, who + "1..8 models");
  GPK_REQUIRE(h, D >= 1 && D <= PROP_MAX_D && nx >= B && nx <= D, who + "the state dimension nx must be in [B, D], D <= 16");
  GPK_REQUIRE(h, !var_includes_noise || noise, who + "null noise levels");
  GPK_REQUIRE(h, (in_shift == nullptr) == (in_scale == nullptr), who + "in_shift and in_scale go together");
  for (int b = 0; b < B; ++b) GPK_REQUIRE(h, X[b] && alpha[b] && W[b], who + "null model pointer");
  PropK k{};
  k.nx = nx; k.D = D; k.NO = B;
  k.so = R; k.sm = 1; k.vo = R; k.vm = 1;
  k.add_noise = var_includes_noise != 0;
  for (int d = 0; d < 16; ++d) { k.in_shift[d] = 0.0; k.in_scale[d] = 1.0; k.model_of[d] = -1; }
  for (int b = 0; b < B; ++b) {
    GPK_REQUIRE(h, coord[b] >= 0 && coord[b] < nx, who + "coord must be in [0, nx)");
    GPK_REQUIRE(h, k.model_of[coord[b]] < 0, who + "coord must be distinct");
    k.model_of[coord[b]] = b;
    k.ystd2[b] = y_std[b] * y_std[b];
    k.noise[b] = var_includes_noise ? noise[b] : 0.0;
  }
  GPK_REQUIRE(h, prop_finite(kss, B) && prop_finite(k.noise, B) && prop_finite(&floor_, 1), who + "kss, floor and noise must be finite");
  if (in_shift) {
    GPK_REQUIRE(h, prop_finite(in_shift, D) && prop_finite(in_scale, D), who + "the input scaler must not contain NaN or infinity");
    for (int d = 0; d < D; ++d) {
      GPK_REQUIRE(h, in_scale[d] != 0.0, who + "in_scale must be non-zero");
      k.in_shift[d] = in_shift[d];
      k.in_scale[d] = in_scale[d];
    }
    k.scaled = 1;
  }
  const ServeModels m{B, 1, 1, X, alpha, N, D, ls, sf2, y_mean, y_std, {W, nullptr}, Np, ldw, kss, floor_, nullptr};
  const Horizon z{x0, U, lin, Sigma0, Q, x0_rows, u_rows, s_rows, R, H, traj, Sigma, mean, var, jac, order, corr, grad};
  return gpk_propagate_run(h, who, m, k, z);
}

extern "C" int gpk_propagate_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                        const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                        const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                        int var_includes_noise, const double* noise, int nx, const int* coord,
                                        const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                        const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                        const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                        double* jac) {
  return propagate_host_multi_any(h, "propagate_host_multi: ", B, X, alpha, N, D, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_,
                                  var_includes_noise, noise, nx, coord, in_shift, in_scale, x0, x0_rows, U, u_rows, lin, Sigma0, s_rows,
                                  Q, R, H, traj, Sigma, mean, var, jac, 1, nullptr);
}

extern "C" int gpk_propagate2_host_multi(gpk_handle h, int B, const double* const* X, const double* const* alpha, int64_t N, int D,
                                         const double* ls, const double* sf2, const double* y_mean, const double* y_std,
                                         const double* const* W, int64_t Np, int64_t ldw, const double* kss, double floor_,
                                         int var_includes_noise, const double* noise, int nx, const int* coord,
                                         const double* in_shift, const double* in_scale, const double* x0, int x0_rows,
                                         const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                         const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                         double* jac, int order, double* corr) {
  return propagate_host_multi_any(h, "propagate2_host_multi: ", B, X, alpha, N, D, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_,
                                  var_includes_noise, noise, nx, coord, in_shift, in_scale, x0, x0_rows, U, u_rows, lin, Sigma0,
                                  s_rows, Q, R, H, traj, Sigma, mean, var, jac, order, corr);
}

// ... with the gradient of a horizon cost (order 1): the seeds gx, gS and the results dU, dx0, dSigma0 as HorizonGrad describes them
extern "C" int gpk_propagate_grad_host(gpk_handle h, const double* X, const double* alpha, int64_t N, int D, int P, const double* ls,
                                       double sf2, const double* y_mean, const double* y_std, const double* W, int64_t Np,
                                       int64_t ldw, double kss, double floor_, int var_includes_noise, double noise, const double* x0,
                                       int x0_rows, const double* U, int u_rows, const double* lin, const double* Sigma0, int s_rows,
                                       const double* Q, int R, int H, double* traj, double* Sigma, double* mean, double* var,
                                       double* jac, const double* gx, const double* gS, double* dU, double* dx0, double* dSigma0) {
  const HorizonGrad g{gx, gS, dU, dx0, dSigma0};
  return propagate_host_any(h, "propagate_grad_host: ", X, alpha, N, D, P, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_,
                            var_includes_noise, noise, x0, x0_rows, U, u_rows, lin, Sigma0, s_rows, Q, R, H, traj, Sigma, mean, var, jac,
                            1, nullptr, &g);
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
  return propagate_host_multi_any(h, "propagate_grad_host_multi: ", B, X, alpha, N, D, ls, sf2, y_mean, y_std, W, Np, ldw, kss, floor_,
                                  var_includes_noise, noise, nx, coord, in_shift, in_scale, x0, x0_rows, U, u_rows, lin, Sigma0,
                                  s_rows, Q, R, H, traj, Sigma, mean, var, jac, 1, nullptr, &g);
}
