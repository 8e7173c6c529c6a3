/* Posterior function draws (K10) from a plain C caller - no Python, no torch: the fit building blocks (gpk_gram -> gpk_potrf ->
 * gpk_trtri) on hipMalloc'd buffers, then gpk_rff_features -> gpk_paths_prepare -> gpk_paths_step -> gpk_paths_rollout.
 * The pytest wrapper (tests/test_gpu_paths_c_abi.py) writes the problem and the randomness as one flat file of doubles, argv[1]:
 *   [N, D, F, S, P, H, M, sf2, noise + alpha]  ls (D)  y_mean (P)  y_std (P)  X (N x D)  Yn (N x P)  omega (F x D)  phase (F)
 *   W_rand (F x C)  Eps (N x C)  Xs (S x D)  x0 (S x P)  U (H x (D - P))  lin (P x D)  Xq (M x D)            C = S P
 * and compares what this program writes to argv[2] with the dense NumPy form:
 *   Phi (M x F; gpk_rff_features of Xq, scale 0.7)  Coef ((N + F) x C)  step (S x P)  traj ((H + 1) x S x P)
 * The program itself checks the zeros in the padding of Phi, that Coef's pitch columns are left alone, that repeated calls
 * repeat their bits, and every bad-argument status.
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
  const long N = (long)buf[0], F = (long)buf[2], M = (long)buf[6];
  const int D = (int)buf[1], S = (int)buf[3], P = (int)buf[4], H = (int)buf[5];
  const double sf2 = buf[7], s2 = buf[8];
  const long C = (long)S * P, du = D - P;
  const double* ls = buf + 9;
  const double *ym = ls + D, *ys = ym + P, *X = ys + P, *Yn = X + N * D, *omega = Yn + N * P, *phase = omega + F * D;
  const double *Wr = phase + F, *Eps = Wr + F * C, *Xs = Eps + N * C, *x0 = Xs + (long)S * D, *U = x0 + C, *lin = U + H * du;
  const double* Xq = lin + P * D;
  EXPECT((Xq + M * D - buf) * (long)sizeof(double) == bytes && du >= 1, "file layout: %ld bytes", bytes);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  CHECK_GPK(gpk_set_option(h, "debug_fill", 1));
  const int64_t Np = gpk_padded(N), Fp = gpk_padded(F), Mp = gpk_padded(M);
  const int64_t ldc = C + 2;      /* pitched: two columns nobody may touch */
  double *dX = to_device(X, N * D), *dYn = to_device(Yn, N * P), *dOm = to_device(omega, F * D), *dPh = to_device(phase, F);
  double *dWr = to_device(Wr, F * C), *dEps = to_device(Eps, N * C), *dXs = to_device(Xs, (size_t)S * D), *dXq = to_device(Xq, M * D);
  EXPECT(dX && dYn && dOm && dPh && dWr && dEps && dXs && dXq, "device allocation");
  double *dK, *dW, *dtr, *dwinv, *dPhi, *dCoef, *dOut;
  const size_t nK = (size_t)Np * Np, ntr = (size_t)(Np / 2 + 128) * (Np / 2 + 128), nPhi = (size_t)Mp * Fp, nCoef = (size_t)(N + F) * ldc;
  CHECK_HIP(hipMalloc((void**)&dK, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dW, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dtr, sizeof(double) * ntr));
  CHECK_HIP(hipMalloc((void**)&dwinv, sizeof(double) * Np * GPK_TILE));
  CHECK_HIP(hipMalloc((void**)&dPhi, sizeof(double) * nPhi));
  CHECK_HIP(hipMalloc((void**)&dCoef, sizeof(double) * nCoef));
  CHECK_HIP(hipMalloc((void**)&dOut, sizeof(double) * C));
  /* every buffer the library writes starts out as NaN */
  CHECK_HIP(hipMemset(dK, 0xFF, sizeof(double) * nK));
  CHECK_HIP(hipMemset(dW, 0xFF, sizeof(double) * nK));
  CHECK_HIP(hipMemset(dtr, 0xFF, sizeof(double) * ntr));
  CHECK_HIP(hipMemset(dPhi, 0xFF, sizeof(double) * nPhi));
  CHECK_HIP(hipMemset(dCoef, 0xFF, sizeof(double) * nCoef));
  CHECK_HIP(hipMemset(dOut, 0xFF, sizeof(double) * C));

  /* ---- fit: K = k(X, X) + (noise + alpha) I, L, W = L^-1 ----------------------------------------------------------------- */
  int info = -1;
  CHECK_GPK(gpk_gram(h, GPK_F64, dX, N, D, ls, sf2, s2, dK, Np));
  CHECK_GPK(gpk_potrf(h, dK, Np, Np, dwinv, &info));
  EXPECT(info == 0, "potrf info %d", info);
  CHECK_GPK(gpk_trtri(h, dK, Np, Np, dwinv, dW, Np, dtr));

  const size_t nPhiOut = (size_t)M * F, nCoefOut = (size_t)(N + F) * C, nTraj = (size_t)(H + 1) * C;
  const size_t nOut = nPhiOut + nCoefOut + C + nTraj;
  double* out = (double*)malloc(sizeof(double) * nOut);
  double *oPhi = out, *oCoef = oPhi + nPhiOut, *oStep = oCoef + nCoefOut, *oTraj = oStep + C;

  /* ---- gpk_rff_features: the padded block, zeros in the padding ----------------------------------------------------------- */
  CHECK_GPK(gpk_rff_features(h, dXq, M, D, dOm, dPh, F, 0.7, dPhi, Fp));
  CHECK_GPK(gpk_synchronize(h));
  double* hPhi = (double*)malloc(sizeof(double) * nPhi);
  CHECK_HIP(hipMemcpy(hPhi, dPhi, sizeof(double) * nPhi, hipMemcpyDeviceToHost));
  for (long m = 0; m < Mp; ++m)
    for (long k = 0; k < Fp; ++k) {
      const double v = hPhi[m * Fp + k];
      if (m < M && k < F) { EXPECT(fabs(v) <= 0.7, "Phi[%ld][%ld] = %g", m, k, v); oPhi[m * F + k] = v; }
      else EXPECT(v == 0.0, "padding of Phi at [%ld][%ld] = %g", m, k, v);
    }

  /* ---- gpk_paths_prepare into a pitched Coef ------------------------------------------------------------------------------- */
  CHECK_GPK(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc));
  CHECK_GPK(gpk_synchronize(h));
  double* hCoef = (double*)malloc(sizeof(double) * nCoef);
  CHECK_HIP(hipMemcpy(hCoef, dCoef, sizeof(double) * nCoef, hipMemcpyDeviceToHost));
  for (long j = 0; j < N + F; ++j) {
    memcpy(oCoef + j * C, hCoef + j * ldc, sizeof(double) * C);
    for (long c = 0; c < C; ++c) EXPECT(isfinite(hCoef[j * ldc + c]), "Coef[%ld][%ld] is not finite", j, c);
    EXPECT(isnan(hCoef[j * ldc + C]) && isnan(hCoef[j * ldc + C + 1]), "row %ld: the pitch columns were written", j);
  }
  /* once more: the same bits */
  CHECK_GPK(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc));
  CHECK_GPK(gpk_synchronize(h));
  double* again = (double*)malloc(sizeof(double) * (nCoef > nTraj ? nCoef : nTraj));
  CHECK_HIP(hipMemcpy(again, dCoef, sizeof(double) * nCoef, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(again, hCoef, sizeof(double) * nCoef), "gpk_paths_prepare: two calls differ");

  /* ---- gpk_paths_step, twice ----------------------------------------------------------------------------------------------- */
  CHECK_GPK(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(oStep, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemset(dOut, 0xFF, sizeof(double) * C));
  CHECK_GPK(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(again, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(again, oStep, sizeof(double) * C), "gpk_paths_step: two calls differ");
  for (long c = 0; c < C; ++c) EXPECT(isfinite(oStep[c]), "step[%ld] is not finite", c);

  /* ---- gpk_paths_rollout, twice; H = 1 is x0 + lin q + step(q); one start for every path ----------------------------------- */
  for (size_t i = 0; i < nTraj; ++i) oTraj[i] = again[i] = NAN;
  CHECK_GPK(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, oTraj));
  CHECK_GPK(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, again));
  EXPECT(!memcmp(again, oTraj, sizeof(double) * nTraj), "gpk_paths_rollout: two calls differ");
  EXPECT(!memcmp(oTraj, x0, sizeof(double) * C), "stage 0 of the trajectory is not x0");
  for (size_t i = 0; i < nTraj; ++i) EXPECT(isfinite(oTraj[i]), "traj[%zu] is not finite", i);
  {
    double* q = (double*)malloc(sizeof(double) * S * D);
    double* one = (double*)malloc(sizeof(double) * 2 * C);
    for (int s = 0; s < S; ++s) {
      memcpy(q + (long)s * D, x0 + (long)s * P, sizeof(double) * P);
      memcpy(q + (long)s * D + P, U, sizeof(double) * du);
    }
    CHECK_HIP(hipMemcpy(dXs, q, sizeof(double) * S * D, hipMemcpyHostToDevice));
    CHECK_GPK(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut));
    CHECK_GPK(gpk_synchronize(h));
    CHECK_HIP(hipMemcpy(again, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
    CHECK_GPK(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, 1, lin, one));
    double worst = 0.0, scale = 0.0;
    for (int s = 0; s < S; ++s)
      for (int p = 0; p < P; ++p) {
        double a = 0.0;
        for (int d = 0; d < D; ++d) a += lin[p * D + d] * q[(long)s * D + d];
        const double want = x0[(long)s * P + p] + a + again[(long)s * P + p], got = one[C + (long)s * P + p];
        if (fabs(want) > scale) scale = fabs(want);
        if (fabs(got - want) > worst) worst = fabs(got - want);
      }
    EXPECT(worst <= 1e-12 * scale, "H = 1 against x0 + lin q + step(q): %g", worst / scale);
    EXPECT(!memcmp(one + C, oTraj + C, sizeof(double) * C), "stage 1 of H = 1 differs from stage 1 of H = %d", H);
    /* x0_rows = 1: path 0's start for every path; path 0 itself repeats its bits */
    CHECK_GPK(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, 1, U, 1, lin, one));
    for (int s = 0; s < S; ++s) EXPECT(!memcmp(one + (long)s * P, x0, sizeof(double) * P), "broadcast start, path %d", s);
    EXPECT(!memcmp(one + C, oTraj + C, sizeof(double) * P), "broadcast start: path 0 changed");
    free(q); free(one);
  }

  /* ---- bad arguments: statuses, never a fault ------------------------------------------------------------------------------ */
  BAD(gpk_rff_features(NULL, dXq, M, D, dOm, dPh, F, 0.7, dPhi, Fp), "null handle");
  BAD(gpk_rff_features(h, NULL, M, D, dOm, dPh, F, 0.7, dPhi, Fp), "null X");
  BAD(gpk_rff_features(h, dXq, 0, D, dOm, dPh, F, 0.7, dPhi, Fp), "N = 0");
  BAD(gpk_rff_features(h, dXq, M, 0, dOm, dPh, F, 0.7, dPhi, Fp), "D = 0");
  BAD(gpk_rff_features(h, dXq, M, GPK_MAX_D_PREDICT + 1, dOm, dPh, F, 0.7, dPhi, Fp), "D = 17");
  BAD(gpk_rff_features(h, dXq, M, D, dOm, dPh, 0, 0.7, dPhi, Fp), "F = 0");
  BAD(gpk_rff_features(h, dXq, M, D, dOm, dPh, 16385, 0.7, dPhi, 16512), "F = 16385");
  BAD(gpk_rff_features(h, dXq, M, D, dOm, dPh, F, 0.7, dPhi, Fp - 1), "ldp < gpk_padded(F)");
  EXPECT(strstr(gpk_last_error(h), "ldp") != NULL, "message: %s", gpk_last_error(h));
  BAD(gpk_paths_prepare(NULL, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc), "null handle");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, NULL, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc), "null W");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, NULL, dEps, S, dCoef, ldc), "null W_rand");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np + 128, Np + 128, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc), "Np != gpk_padded(N)");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np - 1, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc), "ldw < Np");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, 0, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc), "P = 0");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, GPK_MAX_P + 1, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, 1 << 20), "P = 17");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, 0, dCoef, ldc), "S = 0");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, 4097, dCoef, 1 << 20), "S = 4097");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, 16385, sf2, dWr, dEps, S, dCoef, ldc), "F = 16385");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, 0.0, dWr, dEps, S, dCoef, ldc), "sf2 = 0");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, C - 1), "ldc < C");
  EXPECT(strstr(gpk_last_error(h), "ldc") != NULL, "message: %s", gpk_last_error(h));
  const double bad_ls[16] = {1.0, -1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
  BAD(gpk_paths_step(NULL, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut), "null handle");
  BAD(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, NULL, ldc, S, P, ym, ys, dXs, dOut), "null Coef");
  BAD(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, NULL, dOut), "null queries");
  BAD(gpk_paths_step(h, dX, N, D, NULL, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut), "null ls");
  BAD(gpk_paths_step(h, dX, N, D, bad_ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut), "negative length-scale");
  BAD(gpk_paths_step(h, dX, 0, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut), "N = 0");
  BAD(gpk_paths_step(h, dX, N, 17, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut), "D = 17");
  BAD(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, 0, dCoef, ldc, S, P, ym, ys, dXs, dOut), "F = 0");
  BAD(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, 0, P, ym, ys, dXs, dOut), "S = 0");
  BAD(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, 1 << 20, 4097, P, ym, ys, dXs, dOut), "S = 4097");
  BAD(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, 17, ym, ys, dXs, dOut), "P = 17");
  BAD(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, C - 1, S, P, ym, ys, dXs, dOut), "ldc < C");
  double* one = again;
  BAD(gpk_paths_rollout(NULL, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, one), "null handle");
  BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, NULL, S, U, H, lin, one), "null x0");
  BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, NULL, H, lin, one), "null U with D > P");
  BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, NULL, one), "null lin");
  BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, NULL), "null traj");
  BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, 0, lin, one), "H = 0");
  BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, 257, lin, one), "H = 257");
  BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, 2, U, H, lin, one), "x0 with 2 rows");
  if (P > 1)   /* as a model of P - 1 inputs the state would be larger than the query */
    BAD(gpk_paths_rollout(h, dX, N, P - 1, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, one), "P > D");
  {
    double* bad = (double*)malloc(sizeof(double) * (C + H * du + P * D));
    double *bx = bad, *bu = bx + C, *bl = bu + H * du;
    memcpy(bx, x0, sizeof(double) * C); memcpy(bu, U, sizeof(double) * H * du); memcpy(bl, lin, sizeof(double) * P * D);
    bx[C - 1] = NAN;
    BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, bx, S, U, H, lin, one), "NaN in x0");
    bu[H * du - 1] = INFINITY;
    BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, bu, H, lin, one), "infinity in U");
    bl[0] = -INFINITY;
    BAD(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, bl, one), "infinity in lin");
    EXPECT(strstr(gpk_last_error(h), "NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    free(bad);
  }
  CHECK_GPK(gpk_batch_begin(h, 2));
  BAD(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut), "batched mode");
  BAD(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc), "batched mode");
  CHECK_GPK(gpk_batch_end(h));
  /* the refusals left the path set alone */
  CHECK_GPK(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, one));
  EXPECT(!memcmp(one, oTraj, sizeof(double) * nTraj), "the path set changed under the refused calls");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), nOut, f) != nOut) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  hipFree(dX); hipFree(dYn); hipFree(dOm); hipFree(dPh); hipFree(dWr); hipFree(dEps); hipFree(dXs); hipFree(dXq);
  hipFree(dK); hipFree(dW); hipFree(dtr); hipFree(dwinv); hipFree(dPhi); hipFree(dCoef); hipFree(dOut);
  gpk_destroy(h);
  free(again); free(hCoef); free(hPhi); free(out); free(buf);
  printf("paths from C: OK\n");
  return 0;
}
