// The stage composition that every horizon chain's composing launch shares (propagate_advance_kernel, gpk_propagate.hip;
// the chain half of moments_finish_kernel, gpk_moments.hip).  One workgroup of 256 threads per rollout r, thread (i, j) =
// (tid >> 4, tid & 15); tiles are [16][17] in LDS; sequential, fixed-order sums.  With A (nx x nx) the stage's state Jacobian:
//   x+ = q_x + lin q (+ mu of the output that drives the coordinate),   Sigma+ = A Sigma A^T + the stage's own term + Q
// The lower triangle of Sigma+ is formed and mirrored, so it is symmetric bit for bit.  x and S are updated in place (the
// workgroup alone touches row r of either).  The caller places __syncthreads() between the steps.
#pragma once
#include "gpk_internal.h"

typedef double StageTile[16][17];

// the rollout's query q = [x, u] and Sigma
__device__ __forceinline__ void stage_load(const StageView& v, int nx, int D, int r, int tid, double* q, StageTile& Sg) {
  const int i = tid >> 4, j = tid & 15;
  if (tid < D) q[tid] = tid < nx ? v.x[(long long)r * nx + tid] : v.u[r * v.u_row_stride + (tid - nx)];
  if (i < nx && j < nx) Sg[i][j] = v.S[((long long)r * nx + i) * nx + j];
}

// xn = q_x + lin q + mu[model_of]  (after stage_load and mu)
__device__ __forceinline__ void stage_mean(const StageView& v, const int* model_of, int nx, int D, int tid, const double* q,
                                           const double* mu, double* xn) {
  if (tid < nx) {
    const int o = model_of[tid];
    double a = 0.0;
    for (int d = 0; d < D; ++d) a = __builtin_fma(v.lin[tid * D + d], q[d], a);
    double val = q[tid] + a;
    if (o >= 0) val += mu[o];
    xn[tid] = val;
  }
}

// T = A Sigma
__device__ __forceinline__ void stage_left(int nx, int tid, const StageTile& A, const StageTile& Sg, StageTile& T) {
  const int i = tid >> 4, j = tid & 15;
  if (i < nx && j < nx) {
    double t = 0.0;
    for (int c = 0; c < nx; ++c) t = __builtin_fma(A[i][c], Sg[c][j], t);
    T[i][j] = t;
  }
}

// Sigma+ (i, j <= i) = (T A^T)(i, j), then own(s, i, j) - the stage's own terms, added in its order - then Q; mirrored into S
// and the horizon's slot
template <class Own>
__device__ __forceinline__ void stage_right(const StageView& v, int nx, int r, int tid, const StageTile& T, const StageTile& A,
                                            Own own) {
  const int i = tid >> 4, j = tid & 15;
  if (i < nx && j <= i) {
    double s = 0.0;
    for (int c = 0; c < nx; ++c) s = __builtin_fma(T[i][c], A[j][c], s);
    s = own(s, i, j);
    if (v.Qn) s += v.Qn[i * nx + j];
    const long long at = (long long)r * nx * nx;
    v.S[at + i * nx + j] = s;
    v.S[at + j * nx + i] = s;
    v.sig_next[at + i * nx + j] = s;
    v.sig_next[at + j * nx + i] = s;
  }
}

// x, the horizon's slot and the next stage's scaled query row
__device__ __forceinline__ void stage_store(const StageView& v, int scaled, const double* in_shift, const double* in_scale, int nx,
                                            int D, int r, int tid, const double* xn) {
  if (tid < nx) {
    v.x[(long long)r * nx + tid] = xn[tid];
    v.traj_next[(long long)r * nx + tid] = xn[tid];
  }
  if (v.qnext && tid < D) {
    const double raw = tid < nx ? xn[tid] : v.u_next[r * v.u_row_stride + (tid - nx)];
    v.qnext[(long long)r * D + tid] = scaled ? (raw - in_shift[tid]) / in_scale[tid] : raw;
  }
}
