/* Path gradients (K10) from a plain C caller - no Python, no torch: the fit building blocks on hipMalloc'd buffers, then
 * gpk_paths_prepare -> gpk_paths_step_grad -> gpk_paths_rollout_grad on a single model, and gpk_paths_step_multi_grad on a batch
 * whose pitched, model-major Coef comes from the file (NaN in the padding and pitch columns).
 * The pytest wrapper (tests/test_gpu_paths_grad_c_abi.py) writes one flat file of doubles, argv[1]:
 *   [N, D, F, S, P, H, sf2, noise + alpha]  ls (D)  y_mean (P)  y_std (P)  X (N x D)  Yn (N x P)  omega (F x D)  phase (F)
 *   W_rand (F x C)  Eps (N x C)  Xs (S x D)  x0 (S x P)  U (H x (D - P))  lin (P x D)                                  C = S P
 *   [N2, D2, F2, S2, B, mstride, ldc2]  ls2 (B x D2)  sf2 (B)  shift (B)  scale (B)  X2 (N2 x D2)  omega2 (B x F2 x D2)
 *   phase2 (B x F2)  Coef2 ((N2 + F2) x ldc2)  Xs2 (S2 x D2)
 * and compares what this program writes to argv[2] with the closed form in NumPy:
 *   jac of the step (S x P x D)  jac of the rollout (H x S x P x D)  jac of the batch step (S2 x B x D2)
 * The program itself checks the statuses, that out / traj have the bytes of the plain entries, that repeated calls repeat their
 * bits, and the refusal of a null jac.
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
  if (hipMalloc((void**)&d, sizeof(double) * n) != hipSuccess) return NULL;
  if (hipMemset(d, 0xFF, sizeof(double) * n) != hipSuccess) return NULL;
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
  const int D = (int)buf[1], S = (int)buf[3], P = (int)buf[4], H = (int)buf[5];
  const double sf2 = buf[6], s2 = buf[7];
  const long C = (long)S * P, du = D - P;
  const double* ls = buf + 8;
  const double *ym = ls + D, *ys = ym + P, *X = ys + P, *Yn = X + N * D, *omega = Yn + N * P, *phase = omega + F * D;
  const double *Wr = phase + F, *Eps = Wr + F * C, *Xs = Eps + N * C, *x0 = Xs + (long)S * D, *U = x0 + C, *lin = U + H * du;
  const double* b2 = lin + P * D;
  const long N2 = (long)b2[0], F2 = (long)b2[2], mstride = (long)b2[5], ldc2 = (long)b2[6];
  const int D2 = (int)b2[1], S2 = (int)b2[3], B = (int)b2[4];
  const double *ls2 = b2 + 7, *sf22 = ls2 + B * D2, *shift = sf22 + B, *scale = shift + B, *X2 = scale + B;
  const double *omega2 = X2 + N2 * D2, *phase2 = omega2 + B * F2 * D2, *Coef2 = phase2 + B * F2, *Xs2 = Coef2 + (N2 + F2) * ldc2;
  EXPECT((Xs2 + (long)S2 * D2 - buf) * (long)sizeof(double) == bytes && du >= 1, "file layout: %ld bytes", bytes);
  EXPECT(mstride >= S2 && ldc2 > B * mstride, "the batch's Coef must be pitched");

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  CHECK_GPK(gpk_set_option(h, "debug_fill", 1));
  const int64_t Np = gpk_padded(N);
  const int64_t ldc = C + 2;      /* pitched: two columns nobody may touch */
  double *dX = to_device(X, N * D), *dYn = to_device(Yn, N * P), *dOm = to_device(omega, F * D), *dPh = to_device(phase, F);
  double *dWr = to_device(Wr, F * C), *dEps = to_device(Eps, N * C), *dXs = to_device(Xs, (size_t)S * D);
  EXPECT(dX && dYn && dOm && dPh && dWr && dEps && dXs, "device allocation");
  const size_t nK = (size_t)Np * Np, ntr = (size_t)(Np / 2 + 128) * (Np / 2 + 128), nCoef = (size_t)(N + F) * ldc;
  const size_t nJac = (size_t)C * D, nTraj = (size_t)(H + 1) * C, nRJac = (size_t)H * C * D;
  double *dK = nan_device(nK), *dW = nan_device(nK), *dtr = nan_device(ntr), *dwinv = nan_device((size_t)Np * GPK_TILE);
  double *dCoef = nan_device(nCoef), *dOut = nan_device(C), *dOutG = nan_device(C), *dJac = nan_device(nJac);
  EXPECT(dK && dW && dtr && dwinv && dCoef && dOut && dOutG && dJac, "device allocation");

  /* ---- fit and set-up ------------------------------------------------------------------------------------------------------ */
  int info = -1;
  CHECK_GPK(gpk_gram(h, GPK_F64, dX, N, D, ls, sf2, s2, dK, Np));
  CHECK_GPK(gpk_potrf(h, dK, Np, Np, dwinv, &info));
  EXPECT(info == 0, "potrf info %d", info);
  CHECK_GPK(gpk_trtri(h, dK, Np, Np, dwinv, dW, Np, dtr));
  CHECK_GPK(gpk_paths_prepare(h, dX, N, D, dYn, P, dW, Np, Np, dOm, dPh, F, sf2, dWr, dEps, S, dCoef, ldc));

  const size_t nMJac = (size_t)S2 * B * D2, nOut = nJac + nRJac + nMJac;
  double* out = (double*)malloc(sizeof(double) * nOut);
  double *oJac = out, *oRJac = oJac + nJac, *oMJac = oRJac + nRJac;
  const size_t nTmp = nRJac > nMJac ? nRJac : nMJac;
  double *tmp = (double*)malloc(sizeof(double) * (nTmp > nTraj ? nTmp : nTraj)), *val = (double*)malloc(sizeof(double) * nTraj);
  double* valg = (double*)malloc(sizeof(double) * nTraj);

  /* ---- gpk_paths_step_grad: out has the bytes of gpk_paths_step; twice ------------------------------------------------------ */
  CHECK_GPK(gpk_paths_step(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOut));
  CHECK_GPK(gpk_paths_step_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOutG, dJac));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(val, dOut, sizeof(double) * C, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(valg, dOutG, sizeof(double) * C, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(oJac, dJac, sizeof(double) * nJac, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(val, valg, sizeof(double) * C), "gpk_paths_step_grad: out differs from gpk_paths_step");
  for (size_t i = 0; i < nJac; ++i) EXPECT(isfinite(oJac[i]), "jac[%zu] is not finite", i);
  CHECK_HIP(hipMemset(dOutG, 0xFF, sizeof(double) * C));
  CHECK_HIP(hipMemset(dJac, 0xFF, sizeof(double) * nJac));
  CHECK_GPK(gpk_paths_step_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOutG, dJac));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(valg, dOutG, sizeof(double) * C, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(tmp, dJac, sizeof(double) * nJac, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(val, valg, sizeof(double) * C) && !memcmp(tmp, oJac, sizeof(double) * nJac), "gpk_paths_step_grad: two calls differ");

  /* ---- gpk_paths_rollout_grad: traj has the bytes of gpk_paths_rollout; twice ------------------------------------------------ */
  for (size_t i = 0; i < nTraj; ++i) val[i] = valg[i] = NAN;
  for (size_t i = 0; i < nRJac; ++i) oRJac[i] = tmp[i] = NAN;
  CHECK_GPK(gpk_paths_rollout(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, val));
  CHECK_GPK(gpk_paths_rollout_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, valg, oRJac));
  EXPECT(!memcmp(val, valg, sizeof(double) * nTraj), "gpk_paths_rollout_grad: traj differs from gpk_paths_rollout");
  for (size_t i = 0; i < nRJac; ++i) EXPECT(isfinite(oRJac[i]), "rollout jac[%zu] is not finite", i);
  for (size_t i = 0; i < nTraj; ++i) valg[i] = NAN;
  CHECK_GPK(gpk_paths_rollout_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, valg, tmp));
  EXPECT(!memcmp(val, valg, sizeof(double) * nTraj) && !memcmp(tmp, oRJac, sizeof(double) * nRJac),
         "gpk_paths_rollout_grad: two calls differ");

  /* ---- gpk_paths_step_multi_grad on the pitched batch Coef -------------------------------------------------------------------- */
  const size_t nCoef2 = (size_t)(N2 + F2) * ldc2, nM = (size_t)S2 * B;
  double *dX2 = to_device(X2, N2 * D2), *dOm2 = to_device(omega2, (size_t)B * F2 * D2), *dPh2 = to_device(phase2, (size_t)B * F2);
  double *dCoef2 = to_device(Coef2, nCoef2), *dXs2 = to_device(Xs2, (size_t)S2 * D2);
  double *dM = nan_device(nM), *dMG = nan_device(nM), *dMJ = nan_device(nMJac);
  EXPECT(dX2 && dOm2 && dPh2 && dCoef2 && dXs2 && dM && dMG && dMJ, "device allocation");
  double *mval = (double*)malloc(sizeof(double) * nM), *mvalg = (double*)malloc(sizeof(double) * nM);
  CHECK_GPK(gpk_paths_step_multi(h, dX2, N2, D2, B, ls2, sf22, dOm2, dPh2, F2, dCoef2, ldc2, mstride, S2, shift, scale, dXs2, dM));
  CHECK_GPK(gpk_paths_step_multi_grad(h, dX2, N2, D2, B, ls2, sf22, dOm2, dPh2, F2, dCoef2, ldc2, mstride, S2, shift, scale, dXs2, dMG,
                                      dMJ));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(mval, dM, sizeof(double) * nM, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(mvalg, dMG, sizeof(double) * nM, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(oMJac, dMJ, sizeof(double) * nMJac, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(mval, mvalg, sizeof(double) * nM), "gpk_paths_step_multi_grad: out differs from gpk_paths_step_multi");
  for (size_t i = 0; i < nMJac; ++i) EXPECT(isfinite(oMJac[i]), "batch jac[%zu] is not finite", i);
  CHECK_HIP(hipMemset(dMJ, 0xFF, sizeof(double) * nMJac));
  CHECK_GPK(gpk_paths_step_multi_grad(h, dX2, N2, D2, B, ls2, sf22, dOm2, dPh2, F2, dCoef2, ldc2, mstride, S2, shift, scale, dXs2, dMG,
                                      dMJ));
  CHECK_GPK(gpk_synchronize(h));
  CHECK_HIP(hipMemcpy(tmp, dMJ, sizeof(double) * nMJac, hipMemcpyDeviceToHost));
  EXPECT(!memcmp(tmp, oMJac, sizeof(double) * nMJac), "gpk_paths_step_multi_grad: two calls differ");

  /* ---- bad arguments: statuses, never a fault -------------------------------------------------------------------------------- */
  BAD(gpk_paths_step_grad(NULL, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOutG, dJac), "null handle");
  BAD(gpk_paths_step_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, dXs, dOutG, NULL), "null jac");
  EXPECT(strstr(gpk_last_error(h), "null jac") != NULL, "message: %s", gpk_last_error(h));
  BAD(gpk_paths_step_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, C - 1, S, P, ym, ys, dXs, dOutG, dJac), "ldc < C");
  BAD(gpk_paths_step_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, 17, ym, ys, dXs, dOutG, dJac), "P = 17");
  BAD(gpk_paths_rollout_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, H, lin, valg, NULL), "null jac");
  BAD(gpk_paths_rollout_grad(h, dX, N, D, ls, sf2, dOm, dPh, F, dCoef, ldc, S, P, ym, ys, x0, S, U, 257, lin, valg, tmp), "H = 257");
  BAD(gpk_paths_step_multi_grad(h, dX2, N2, D2, B, ls2, sf22, dOm2, dPh2, F2, dCoef2, ldc2, mstride, S2, shift, scale, dXs2, dMG, NULL),
      "null jac");
  BAD(gpk_paths_step_multi_grad(h, dX2, N2, D2, 9, ls2, sf22, dOm2, dPh2, F2, dCoef2, ldc2, mstride, S2, shift, scale, dXs2, dMG, dMJ),
      "B = 9");
  BAD(gpk_paths_step_multi_grad(h, dX2, N2, D2, B, ls2, sf22, dOm2, dPh2, F2, dCoef2, ldc2, S2 - 1, S2, shift, scale, dXs2, dMG, dMJ),
      "mstride < S");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), nOut, f) != nOut) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  hipFree(dX); hipFree(dYn); hipFree(dOm); hipFree(dPh); hipFree(dWr); hipFree(dEps); hipFree(dXs);
  hipFree(dK); hipFree(dW); hipFree(dtr); hipFree(dwinv); hipFree(dCoef); hipFree(dOut); hipFree(dOutG); hipFree(dJac);
  hipFree(dX2); hipFree(dOm2); hipFree(dPh2); hipFree(dCoef2); hipFree(dXs2); hipFree(dM); hipFree(dMG); hipFree(dMJ);
  gpk_destroy(h);
  free(tmp); free(val); free(valg); free(mval); free(mvalg); free(out); free(buf);
  printf("path gradients from C: OK\n");
  return 0;
}
