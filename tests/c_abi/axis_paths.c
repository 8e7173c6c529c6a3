/* Posterior function draws of the per-axis batch (K10) from a plain C caller - no Python, no torch: per model the fit building
 * blocks (gpk_gram -> gpk_potrf -> gpk_trtri) and gpk_paths_prepare (P = 1) into that model's column block of ONE pitched
 * coefficient matrix, then gpk_paths_step_multi -> gpk_paths_rollout_multi.
 * The pytest wrapper (tests/test_gpu_axis_paths_c_abi.py) writes the problem and the randomness as one flat file of doubles,
 * argv[1]:
 *   [N, D, F, S, B, H, nx]  sf2 (B)  noise + alpha (B)  shift (B)  scale (B)  ls (B x D)  X (N x D)  Yn (B x N)  omega (B x F x D)
 *   phase (B x F)  W_rand (B x F x S)  Eps (B x N x S)  Xs (S x D)  x0 (S x nx)  U (H x (D - nx))  lin (nx x D)  coord (B)
 *   in_shift (D)  in_scale (D)
 * and compares what this program writes to argv[2] with the dense NumPy form:
 *   Coef blocks ((N + F) x B x S)  step (S x B)  traj ((H + 1) x S x nx)
 * Coef is allocated with mstride = S rounded up to a multiple of 8 and ldc = B mstride + 3, filled with NaN: the program itself
 * checks that the padding between the blocks and the pitch columns are still NaN after every call, that repeated calls repeat
 * their bits, that stage 1 of the rollout is x0 + lin q + step(z), and a bad-argument status of each entry.
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define CHECK_GPK(x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(h)); return 3; } } while (0)
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 4; } } while (0)
#define BAD(call, what) EXPECT((call) == GPK_BAD_ARG, what)

static double* to_device(const double* src, size_t n) {
  double* d = NULL;
  if (hipMalloc((void**)&d, sizeof(double) * (n ? n : 1)) != hipSuccess) return NULL;
  if (n && hipMemcpy(d, src, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) return NULL;
  return d;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <input file> <output file>\n", argv[0]); return 1; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  double* buf = (double*)malloc(bytes);
  if (fread(buf, 1, bytes, f) != (size_t)bytes) { fprintf(stderr, "short read\n"); return 1; }
  fclose(f);
  const long N = (long)buf[0], F = (long)buf[2];
  const int D = (int)buf[1], S = (int)buf[3], B = (int)buf[4], H = (int)buf[5], nx = (int)buf[6];
  EXPECT(B >= 1 && B <= 8 && nx >= B && nx < D, "header: B = %d, nx = %d, D = %d", B, nx, D);
  const long du = D - nx;
  const double *sf2 = buf + 7, *s2 = sf2 + B, *shift = s2 + B, *scale = shift + B, *ls = scale + B, *X = ls + B * D;
  const double *Yn = X + N * D, *omega = Yn + B * N, *phase = omega + B * F * D, *Wr = phase + B * F, *Eps = Wr + B * F * S;
  const double *Xs = Eps + B * N * S, *x0 = Xs + (long)S * D, *U = x0 + (long)S * nx, *lin = U + H * du, *coordf = lin + nx * D;
  const double *in_shift = coordf + B, *in_scale = in_shift + D;
  EXPECT((in_scale + D - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  int coord[8];
  for (int b = 0; b < B; ++b) coord[b] = (int)coordf[b];

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  CHECK_GPK(gpk_set_option(h, "debug_fill", 1));
  const int64_t Np = gpk_padded(N);
  const int64_t mstride = (S + 7) / 8 * 8, ldc = B * mstride + 3;      /* pitched: three columns nobody may touch */
  const long C = (long)S * B, Cx = (long)S * nx;
  double *dX = to_device(X, N * D), *dYn = to_device(Yn, B * N), *dOm = to_device(omega, B * F * D), *dPh = to_device(phase, B * F);
  double *dWr = to_device(Wr, B * F * S), *dEps = to_device(Eps, B * N * S), *dXs = to_device(Xs, (size_t)S * D);
  EXPECT(dX && dYn && dOm && dPh && dWr && dEps && dXs, "device allocation");
  double *dK, *dW, *dtr, *dwinv, *dCoef, *dOut;
  const size_t nK = (size_t)Np * Np, ntr = (size_t)(Np / 2 + 128) * (Np / 2 + 128), nCoef = (size_t)(N + F) * ldc;
  CHECK_HIP(hipMalloc((void**)&dK, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dW, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dtr, sizeof(double) * ntr));
  CHECK_HIP(hipMalloc((void**)&dwinv, sizeof(double) * Np * GPK_TILE));
  CHECK_HIP(hipMalloc((void**)&dCoef, sizeof(double) * nCoef));
  CHECK_HIP(hipMalloc((void**)&dOut, sizeof(double) * C));
  /* every buffer the library writes starts out as NaN */
  CHECK_HIP(hipMemset(dCoef, 0xFF, sizeof(double) * nCoef));
  CHECK_HIP(hipMemset(dOut, 0xFF, sizeof(double) * C));

  /* ---- per model: K_b = k_b(X, X) + (noise_b + alpha) I, L, W = L^-1, then the set-up into the model's column block --------- */
  for (int b = 0; b < B; ++b) {
    int info = -1;
    CHECK_HIP(hipMemset(dK, 0xFF, sizeof(double) * nK));
    CHECK_HIP(hipMemset(dW, 0xFF, sizeof(double) * nK));
    CHECK_HIP(hipMemset(dtr, 0xFF, sizeof(double) * ntr));
    CHECK_GPK(gpk_gram(h, GPK_F64, dX, N, D, ls + b * D, sf2[b], s2[b], dK, Np));
    CHECK_GPK(gpk_potrf(h, dK, Np, Np, dwinv, &info));
    EXPECT(info == 0, "potrf info %d (model %d)", info, b);
    CHECK_GPK(gpk_trtri(h, dK, Np, Np, dwinv, dW, Np, dtr));
    CHECK_GPK(gpk_paths_prepare(h, dX, N, D, dYn + b * N, 1, dW, Np, Np, dOm + b * F * D, dPh + b * F, F, sf2[b], dWr + b * F * S,
                                dEps + b * N * S, S, dCoef + b * mstride, ldc));
    CHECK_GPK(gpk_synchronize(h));
  }

  const size_t nCoefOut = (size_t)(N + F) * C, nTraj = (size_t)(H + 1) * Cx;
  const size_t nOut = nCoefOut + C + nTraj;
  double* out = (double*)malloc(sizeof(double) * nOut);
  double *oCoef = out, *oStep = oCoef + nCoefOut, *oTraj = oStep + C;
  double* hCoef = (double*)malloc(sizeof(double) * nCoef);
  double* again = (double*)malloc(sizeof(double) * (nCoef > nTraj ? nCoef : nTraj));
  CHECK_HIP(hipMemcpy(hCoef, dCoef, sizeof(double) * nCoef, hipMemcpyDeviceToHost));
  for (long j = 0; j < N + F; ++j)
    for (long c = 0; c < ldc; ++c) {
      const double v = hCoef[j * ldc + c];
      const long b = c / mstride, s = c % mstride;
      if (b < B && s < S) { EXPECT(isfinite(v), "Coef[%ld][%ld] is not finite", j, c); oCoef[j * C + b * S + s] = v; }
      else EXPECT(isnan(v), "row %ld: column %ld (padding or pitch) was written", j, c);
    }

  /* ---- gpk_paths_step_multi, twice ----------------------------------------------------------------------------------------- */
  CHECK_GPK(gpk_paths_step_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(oStep, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemset(dOut, 0xFF, sizeof(double) * C));
  CHECK_GPK(gpk_paths_step_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(again, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(again, oStep, sizeof(double) * C), "gpk_paths_step_multi: two calls differ");
  for (long c = 0; c < C; ++c) EXPECT(isfinite(oStep[c]), "step[%ld] is not finite", c);

  /* ---- gpk_paths_rollout_multi, twice; stage 1 is x0 + lin q + step(z); one start for every path --------------------------- */
  for (size_t i = 0; i < nTraj; ++i) oTraj[i] = again[i] = NAN;
  CHECK_GPK(gpk_paths_rollout_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord, in_shift,
                                    in_scale, x0, S, U, H, lin, oTraj));
  CHECK_GPK(gpk_paths_rollout_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord, in_shift,
                                    in_scale, x0, S, U, H, lin, again));
  EXPECT(!memcmp(again, oTraj, sizeof(double) * nTraj), "gpk_paths_rollout_multi: two calls differ");
  EXPECT(!memcmp(oTraj, x0, sizeof(double) * Cx), "stage 0 of the trajectory is not x0");
  for (size_t i = 0; i < nTraj; ++i) EXPECT(isfinite(oTraj[i]), "traj[%zu] is not finite", i);
  {
    double* q = (double*)malloc(sizeof(double) * S * D);
    double* z = (double*)malloc(sizeof(double) * S * D);
    double* one = (double*)malloc(sizeof(double) * 2 * Cx);
    for (int s = 0; s < S; ++s) {
      memcpy(q + (long)s * D, x0 + (long)s * nx, sizeof(double) * nx);
      memcpy(q + (long)s * D + nx, U, sizeof(double) * du);
      for (int d = 0; d < D; ++d) z[(long)s * D + d] = (q[(long)s * D + d] - in_shift[d]) / in_scale[d];
    }
    CHECK_HIP(hipMemcpy(dXs, z, sizeof(double) * S * D, hipMemcpyHostToDevice));
    CHECK_GPK(gpk_paths_step_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut));
    CHECK_GPK(gpk_synchronize(h));
    CHECK_HIP(hipMemcpy(again, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
    double worst = 0.0, big = 0.0;
    for (int s = 0; s < S; ++s)
      for (int i = 0; i < nx; ++i) {
        double a = 0.0;
        for (int d = 0; d < D; ++d) a += lin[i * D + d] * q[(long)s * D + d];
        double want = x0[(long)s * nx + i] + a;
        for (int b = 0; b < B; ++b)
          if (coord[b] == i) want += again[(long)s * B + b];
        const double got = oTraj[Cx + (long)s * nx + i];
        if (fabs(want) > big) big = fabs(want);
        if (fabs(got - want) > worst) worst = fabs(got - want);
      }
    EXPECT(worst <= 1e-12 * big, "stage 1 against x0 + lin q + step(z): %g", worst / big);
    /* x0_rows = 1: path 0's start for every path; path 0 itself repeats its bits */
    CHECK_GPK(gpk_paths_rollout_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord,
                                      in_shift, in_scale, x0, 1, U, 1, lin, one));
    for (int s = 0; s < S; ++s) EXPECT(!memcmp(one + (long)s * nx, x0, sizeof(double) * nx), "broadcast start, path %d", s);
    EXPECT(!memcmp(one + Cx, oTraj + Cx, sizeof(double) * nx), "broadcast start: path 0 changed");
    free(q); free(z); free(one);
  }

  /* ---- bad arguments: statuses, never a fault; Coef untouched by everything above ---------------------------------------------- */
  BAD(gpk_paths_step_multi(NULL, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut), "null handle");
  BAD(gpk_paths_step_multi(h, dX, N, D, 9, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut), "B = 9");
  BAD(gpk_paths_step_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, S - 1, S, shift, scale, dXs, dOut), "mstride < S");
  EXPECT(strstr(gpk_last_error(h), "mstride") != NULL, "message: %s", gpk_last_error(h));
  BAD(gpk_paths_step_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, B * mstride - 1, mstride, S, shift, scale, dXs, dOut), "ldc");
  EXPECT(strstr(gpk_last_error(h), "ldc") != NULL, "message: %s", gpk_last_error(h));
  {
    int twice[8] = {0};
    BAD(gpk_paths_rollout_multi(NULL, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord, in_shift,
                                in_scale, x0, S, U, H, lin, again), "null handle");
    BAD(gpk_paths_rollout_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, B > 1 ? twice : NULL,
                                in_shift, in_scale, x0, S, U, H, lin, again), "coord twice the same");
    BAD(gpk_paths_rollout_multi(h, dX, N, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord, in_shift,
                                in_scale, x0, S, U, 257, lin, again), "H = 257");
    EXPECT(strstr(gpk_last_error(h), "H must be") != NULL, "message: %s", gpk_last_error(h));
  }
  CHECK_HIP(hipMemcpy(again, dCoef, sizeof(double) * nCoef, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(again, hCoef, sizeof(double) * nCoef), "the coefficient matrix changed");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), nOut, f) != nOut) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  hipFree(dX); hipFree(dYn); hipFree(dOm); hipFree(dPh); hipFree(dWr); hipFree(dEps); hipFree(dXs);
  hipFree(dK); hipFree(dW); hipFree(dtr); hipFree(dwinv); hipFree(dCoef); hipFree(dOut);
  gpk_destroy(h);
  free(again); free(hCoef); free(out); free(buf);
  printf("axis paths from C: OK\n");
  return 0;
}
