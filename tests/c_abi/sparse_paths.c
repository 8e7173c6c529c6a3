/* Posterior function draws of the sparse models (K10, "the sparse models") from a plain C caller - no Python, no torch.
 * Part 1, one model with P outputs: gpk_sparse_begin -> gpk_sparse_update -> gpk_sparse_finalize -> gpk_sparse_paths_prepare into
 * a pitched coefficient matrix -> gpk_paths_step on the copy of Z the set-up wrote.  Part 2, B single-output models without rows
 * (the prior), a handle each: gpk_sparse_begin -> gpk_sparse_finalize -> gpk_sparse_paths_prepare into that model's column block of
 * ONE pitched coefficient matrix and its slice of Zs, then gpk_paths_step_multi_z -> gpk_paths_rollout_multi_z on the first handle.
 * The pytest wrapper (tests/test_gpu_sparse_paths_c_abi.py) writes two flat files of doubles,
 *   argv[1]: [m, D, F, S, P, n]  hyper (4: sf2, noise, alpha, jitter_uu)  y_mean (P)  y_std (P)  ls (D)  Z (m x D)  X (n x D)
 *            Y (n x P)  omega (F x D)  phase (F)  W_rand (F x S P)  Xi (m x S P)  Xs (S x D)
 *   argv[2]: [m, D, F, S, B, H, nx]  hyper (B x 4)  y_mean (B)  y_std (B)  shift (B)  scale (B)  ls (B x D)  Z (B x m x D)
 *            omega (B x F x D)  phase (B x F)  W_rand (B x F x S)  Xi (B x m x S)  Xs (S x D)  x0 (S x nx)  U (H x (D - nx))
 *            lin (nx x D)  coord (B)  in_shift (D)  in_scale (D)
 * and compares what this program writes to argv[3] with the dense NumPy form:
 *   Coef ((m + F) x S P)  step (S x P)  |  Coef blocks ((m + F) x B x S)  Zs (B x m x D)  step (S x B)  traj ((H + 1) x S x nx)
 * Both coefficient matrices are pitched (ldc = C + 3, ldc = B mstride + 3) and filled with NaN: the program itself checks that
 * the padding between the blocks and the pitch columns are still NaN after every call, that repeated calls repeat their bits, and
 * a bad-argument status of each new entry.
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

static double* nan_device(size_t n) {
  double* d = NULL;
  if (hipMalloc((void**)&d, sizeof(double) * (n ? n : 1)) != hipSuccess) return NULL;
  if (hipMemset(d, 0xFF, sizeof(double) * (n ? n : 1)) != hipSuccess) return NULL;
  return d;
}

static double* read_file(const char* path, long* bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return NULL; }
  fseek(f, 0, SEEK_END);
  *bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  double* buf = (double*)malloc(*bytes);
  if (fread(buf, 1, *bytes, f) != (size_t)*bytes) { fprintf(stderr, "short read\n"); return NULL; }
  fclose(f);
  return buf;
}

static gpk_handle new_handle(void) {
  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) return NULL;
  if (gpk_set_stream(h, GPK_OWN_STREAM) != GPK_OK || gpk_set_option(h, "debug_fill", 1) != GPK_OK) return NULL;
  return h;
}

/* part 1: appends Coef ((m + F) x C) and step (S x P) to out */
static int single_model(const double* buf, long bytes, FILE* out) {
  const long m = (long)buf[0], F = (long)buf[2], n = (long)buf[5];
  const int D = (int)buf[1], S = (int)buf[3], P = (int)buf[4];
  const long C = (long)S * P, ldc = C + 3;      /* pitched: three columns nobody may touch */
  const double *hyper = buf + 6, *ym = hyper + 4, *ys = ym + P, *ls = ys + P, *Z = ls + D, *X = Z + m * D, *Y = X + n * D;
  const double *omega = Y + n * P, *phase = omega + F * D, *Wr = phase + F, *Xi = Wr + F * C, *Xs = Xi + m * C;
  EXPECT((Xs + (long)S * D - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  gpk_handle h = new_handle();
  EXPECT(h != NULL, "gpk_create");
  double *dOm = to_device(omega, F * D), *dPh = to_device(phase, F), *dWr = to_device(Wr, F * C), *dXi = to_device(Xi, m * C);
  double *dXs = to_device(Xs, (size_t)S * D), *dCoef = nan_device((m + F) * ldc), *dZ = nan_device(m * D), *dOut = nan_device(C);
  EXPECT(dOm && dPh && dWr && dXi && dXs && dCoef && dZ && dOut, "device allocation");
  CHECK_GPK(gpk_sparse_begin(h, Z, m, D, P, ls, D, hyper[0], hyper[1], hyper[2], hyper[3], ym, ys));
  /* not assembled yet: a status, and nothing written */
  BAD(gpk_sparse_paths_prepare(h, dOm, dPh, F, dWr, dXi, S, dCoef, ldc, dZ), "a model that is not assembled");
  EXPECT(strstr(gpk_last_error(h), "finalised") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(gpk_sparse_update(h, X, Y, n));
  int info = -1;
  CHECK_GPK(gpk_sparse_finalize(h, &info));
  EXPECT(info == 0, "finalize info %d", info);
  BAD(gpk_sparse_paths_prepare(NULL, dOm, dPh, F, dWr, dXi, S, dCoef, ldc, dZ), "null handle");
  BAD(gpk_sparse_paths_prepare(h, dOm, dPh, F, dWr, dXi, S, dCoef, C - 1, dZ), "ldc < C");
  EXPECT(strstr(gpk_last_error(h), "ldc") != NULL, "message: %s", gpk_last_error(h));
  BAD(gpk_sparse_paths_prepare(h, dOm, dPh, 16385, dWr, dXi, S, dCoef, ldc, dZ), "F = 16385");
  BAD(gpk_sparse_paths_prepare(h, dOm, dPh, F, dWr, dXi, 4097, dCoef, 4097 * (long)P, dZ), "S = 4097");
  BAD(gpk_sparse_paths_prepare(h, dOm, dPh, F, dWr, dXi, S, dCoef, ldc, NULL), "null Zdst");
  CHECK_GPK(gpk_synchronize(h));
  double* hCoef = (double*)malloc(sizeof(double) * (m + F) * ldc);
  double* hZ = (double*)malloc(sizeof(double) * m * D);
  CHECK_HIP(hipMemcpy(hCoef, dCoef, sizeof(double) * (m + F) * ldc, hipMemcpyDeviceToHost));
  for (long i = 0; i < (m + F) * ldc; ++i) EXPECT(isnan(hCoef[i]), "a refused set-up wrote Coef[%ld]", i);
  CHECK_GPK(gpk_sparse_paths_prepare(h, dOm, dPh, F, dWr, dXi, S, dCoef, ldc, dZ));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(hCoef, dCoef, sizeof(double) * (m + F) * ldc, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hZ, dZ, sizeof(double) * m * D, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(hZ, Z, sizeof(double) * m * D), "Zdst is not the model's inducing inputs");
  double* res = (double*)malloc(sizeof(double) * ((m + F) * C + C));
  for (long j = 0; j < m + F; ++j)
    for (long c = 0; c < ldc; ++c) {
      const double v = hCoef[j * ldc + c];
      if (c < C) { EXPECT(isfinite(v), "Coef[%ld][%ld] is not finite", j, c); res[j * C + c] = v; }
      else EXPECT(isnan(v), "row %ld: pitch column %ld was written", j, c);
    }
  double *step = res + (m + F) * C, *again = (double*)malloc(sizeof(double) * C);
  CHECK_GPK(gpk_paths_step(h, dZ, m, D, ls, hyper[0], dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(step, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemset(dOut, 0xFF, sizeof(double) * C));
  CHECK_GPK(gpk_paths_step(h, dZ, m, D, ls, hyper[0], dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(again, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(again, step, sizeof(double) * C), "gpk_paths_step: two calls differ");
  for (long c = 0; c < C; ++c) EXPECT(isfinite(step[c]), "step[%ld] is not finite", c);
  if (fwrite(res, sizeof(double), (m + F) * C + C, out) != (size_t)((m + F) * C + C)) { fprintf(stderr, "short write\n"); return 1; }
  hipFree(dOm); hipFree(dPh); hipFree(dWr); hipFree(dXi); hipFree(dXs); hipFree(dCoef); hipFree(dZ); hipFree(dOut);
  gpk_destroy(h);
  free(hCoef); free(hZ); free(res); free(again);
  return 0;
}

/* part 2: appends the Coef blocks ((m + F) x B x S), Zs (B x m x D), step (S x B) and traj ((H + 1) x S x nx) to out */
static int batch(const double* buf, long bytes, FILE* out) {
  const long m = (long)buf[0], F = (long)buf[2];
  const int D = (int)buf[1], S = (int)buf[3], B = (int)buf[4], H = (int)buf[5], nx = (int)buf[6];
  EXPECT(B >= 1 && B <= 8 && nx >= B && nx < D, "header: B = %d, nx = %d, D = %d", B, nx, D);
  const long du = D - nx;
  const double *hyper = buf + 7, *ym = hyper + 4 * B, *ys = ym + B, *shift = ys + B, *scale = shift + B, *ls = scale + B;
  const double *Z = ls + B * D, *omega = Z + B * m * D, *phase = omega + B * F * D, *Wr = phase + B * F, *Xi = Wr + B * F * S;
  const double *Xs = Xi + B * m * S, *x0 = Xs + (long)S * D, *U = x0 + (long)S * nx, *lin = U + H * du, *coordf = lin + nx * D;
  const double *in_shift = coordf + B, *in_scale = in_shift + D;
  EXPECT((in_scale + D - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  int coord[8];
  double sf2[8];
  for (int b = 0; b < B; ++b) { coord[b] = (int)coordf[b]; sf2[b] = hyper[4 * b]; }
  const int64_t mstride = (S + 7) / 8 * 8, ldc = B * mstride + 3;      /* pitched: three columns nobody may touch */
  const long C = (long)S * B, Cx = (long)S * nx;
  const size_t nCoef = (size_t)(m + F) * ldc;
  double *dOm = to_device(omega, B * F * D), *dPh = to_device(phase, B * F), *dWr = to_device(Wr, B * F * S);
  double *dXi = to_device(Xi, B * m * S), *dXs = to_device(Xs, (size_t)S * D);
  double *dCoef = nan_device(nCoef), *dZs = nan_device(B * m * D), *dOut = nan_device(C);
  EXPECT(dOm && dPh && dWr && dXi && dXs && dCoef && dZs && dOut, "device allocation");
  gpk_handle hs[8] = {0};
  gpk_handle h = NULL;
  /* ---- per model: its own handle, the prior (no rows) assembled, the set-up into the model's column block and slice of Zs ---- */
  for (int b = 0; b < B; ++b) {
    h = hs[b] = new_handle();
    EXPECT(h != NULL, "gpk_create (model %d)", b);
    int info = -1;
    CHECK_GPK(gpk_sparse_begin(h, Z + b * m * D, m, D, 1, ls + b * D, D, hyper[4 * b], hyper[4 * b + 1], hyper[4 * b + 2],
                               hyper[4 * b + 3], ym + b, ys + b));
    CHECK_GPK(gpk_sparse_finalize(h, &info));
    EXPECT(info == 0, "finalize info %d (model %d)", info, b);
    CHECK_GPK(gpk_sparse_paths_prepare(h, dOm + b * F * D, dPh + b * F, F, dWr + b * F * S, dXi + b * m * S, S, dCoef + b * mstride,
                                       ldc, dZs + b * m * D));
    CHECK_GPK(gpk_synchronize(h));
  }
  h = hs[0];
  const size_t nCoefOut = (size_t)(m + F) * C, nZ = (size_t)B * m * D, nTraj = (size_t)(H + 1) * Cx;
  const size_t nOut = nCoefOut + nZ + C + nTraj;
  double* res = (double*)malloc(sizeof(double) * nOut);
  double *oCoef = res, *oZ = oCoef + nCoefOut, *oStep = oZ + nZ, *oTraj = oStep + C;
  double* hCoef = (double*)malloc(sizeof(double) * nCoef);
  double* again = (double*)malloc(sizeof(double) * (nCoef > nTraj ? nCoef : nTraj));
  CHECK_HIP(hipMemcpy(hCoef, dCoef, sizeof(double) * nCoef, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(oZ, dZs, sizeof(double) * nZ, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(oZ, Z, sizeof(double) * nZ), "Zs is not the models' inducing inputs");
  for (long j = 0; j < m + F; ++j)
    for (long c = 0; c < ldc; ++c) {
      const double v = hCoef[j * ldc + c];
      const long b = c / mstride, s = c % mstride;
      if (b < B && s < S) { EXPECT(isfinite(v), "Coef[%ld][%ld] is not finite", j, c); oCoef[j * C + b * S + s] = v; }
      else EXPECT(isnan(v), "row %ld: column %ld (padding or pitch) was written", j, c);
    }

  /* ---- gpk_paths_step_multi_z, twice ------------------------------------------------------------------------------------------ */
  CHECK_GPK(gpk_paths_step_multi_z(h, dZs, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(oStep, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemset(dOut, 0xFF, sizeof(double) * C));
  CHECK_GPK(gpk_paths_step_multi_z(h, dZs, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(again, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(again, oStep, sizeof(double) * C), "gpk_paths_step_multi_z: two calls differ");
  for (long c = 0; c < C; ++c) EXPECT(isfinite(oStep[c]), "step[%ld] is not finite", c);

  /* ---- gpk_paths_rollout_multi_z, twice ---------------------------------------------------------------------------------------- */
  for (size_t i = 0; i < nTraj; ++i) oTraj[i] = again[i] = NAN;
  CHECK_GPK(gpk_paths_rollout_multi_z(h, dZs, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord,
                                      in_shift, in_scale, x0, S, U, H, lin, oTraj));
  CHECK_GPK(gpk_paths_rollout_multi_z(h, dZs, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord,
                                      in_shift, in_scale, x0, S, U, H, lin, again));
  EXPECT(!memcmp(again, oTraj, sizeof(double) * nTraj), "gpk_paths_rollout_multi_z: two calls differ");
  EXPECT(!memcmp(oTraj, x0, sizeof(double) * Cx), "stage 0 of the trajectory is not x0");
  for (size_t i = 0; i < nTraj; ++i) EXPECT(isfinite(oTraj[i]), "traj[%zu] is not finite", i);

  /* ---- bad arguments: statuses, never a fault; Coef untouched by everything above -------------------------------------------- */
  BAD(gpk_paths_step_multi_z(NULL, dZs, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut), "null handle");
  BAD(gpk_paths_step_multi_z(h, NULL, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut), "null Zs");
  BAD(gpk_paths_step_multi_z(h, dZs, m, D, 9, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, dXs, dOut), "B = 9");
  BAD(gpk_paths_step_multi_z(h, dZs, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, S - 1, S, shift, scale, dXs, dOut), "mstride < S");
  EXPECT(strstr(gpk_last_error(h), "mstride") != NULL, "message: %s", gpk_last_error(h));
  BAD(gpk_paths_rollout_multi_z(NULL, dZs, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord, in_shift,
                                in_scale, x0, S, U, H, lin, again), "null handle");
  BAD(gpk_paths_rollout_multi_z(h, dZs, m, D, B, ls, sf2, dOm, dPh, F, dCoef, ldc, mstride, S, shift, scale, nx, coord, in_shift,
                                in_scale, x0, S, U, 257, lin, again), "H = 257");
  EXPECT(strstr(gpk_last_error(h), "H must be") != NULL, "message: %s", gpk_last_error(h));
  CHECK_HIP(hipMemcpy(again, dCoef, sizeof(double) * nCoef, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(again, hCoef, sizeof(double) * nCoef), "the coefficient matrix changed");

  if (fwrite(res, sizeof(double), nOut, out) != nOut) { fprintf(stderr, "short write\n"); return 1; }
  hipFree(dOm); hipFree(dPh); hipFree(dWr); hipFree(dXi); hipFree(dXs); hipFree(dCoef); hipFree(dZs); hipFree(dOut);
  for (int b = 0; b < B; ++b) gpk_destroy(hs[b]);
  free(again); free(hCoef); free(res);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <single input> <batch input> <output file>\n", argv[0]); return 1; }
  long b1 = 0, b2 = 0;
  double *in1 = read_file(argv[1], &b1), *in2 = read_file(argv[2], &b2);
  if (!in1 || !in2) return 1;
  FILE* out = fopen(argv[3], "wb");
  if (!out) { perror(argv[3]); return 1; }
  int rc = single_model(in1, b1, out);
  if (rc == 0) rc = batch(in2, b2, out);
  fclose(out);
  free(in1); free(in2);
  if (rc) return rc;
  printf("sparse paths from C: OK\n");
  return 0;
}
