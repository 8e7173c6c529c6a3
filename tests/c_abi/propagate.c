/* Horizon propagation (K11) from a plain C caller - no Python, no torch: the fit building blocks (gpk_gram -> gpk_potrf ->
 * gpk_trtri -> gpk_potrs_inv) on hipMalloc'd buffers, then gpk_propagate_host on the model with P outputs and
 * gpk_propagate_host_multi on the same outputs as B = P single-output models behind an input scaler.
 * The pytest wrapper (tests/test_gpu_propagate_c_abi.py) writes the problem as one flat file of doubles, argv[1]:
 *   [N, D, P, R, H, sf2, noise, alpha]  ls (D)  y_mean (P)  y_std (P)  X (N x D)  Yn (N x P)  YnT (P x N)  x0 (R x P)
 *   U (R x H x (D - P))  lin (P x D)  Sigma0 (P x P)  Q (P x P)  in_shift (D)  in_scale (D)
 * and compares what this program writes to argv[2] with the dense NumPy form:
 *   single: traj ((H + 1) x R x P)  Sigma ((H + 1) x R x P x P)  mean (H x R x P)  var (H x R x P)  jac (H x R x P x D)
 *   multi:  the same five blocks (latent variances + the noise level through var_includes_noise, the scaled queries)
 * The program itself checks that repeated calls repeat their bits, that NULL stage outputs change nothing, that Sigma is symmetric
 * bit for bit, and every bad-argument status.
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
  const long N = (long)buf[0];
  const int D = (int)buf[1], P = (int)buf[2], R = (int)buf[3], H = (int)buf[4];
  const double sf2 = buf[5], noise = buf[6], alpha_j = buf[7];
  const long nu = D - P;
  const double* ls = buf + 8;
  const double *ym = ls + D, *ys = ym + P, *X = ys + P, *Yn = X + N * D, *YnT = Yn + N * P, *x0 = YnT + N * P;
  const double *U = x0 + (long)R * P, *lin = U + (long)R * H * nu, *S0 = lin + P * D, *Q = S0 + P * P, *ish = Q + P * P, *isc = ish + D;
  EXPECT((isc + D - buf) * (long)sizeof(double) == bytes && nu >= 1 && P >= 2 && P <= 8, "file layout: %ld bytes", bytes);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  CHECK_GPK(gpk_set_option(h, "debug_fill", 1));
  const int64_t Np = gpk_padded(N);
  double *dX = to_device(X, N * D), *dYn = to_device(Yn, N * P), *dYnT = to_device(YnT, N * P);
  EXPECT(dX && dYn && dYnT, "device allocation");
  double *dK, *dW, *dtr, *dwinv, *dA, *dAT;
  const size_t nK = (size_t)Np * Np, ntr = (size_t)(Np / 2 + 128) * (Np / 2 + 128);
  CHECK_HIP(hipMalloc((void**)&dK, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dW, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dtr, sizeof(double) * ntr));
  CHECK_HIP(hipMalloc((void**)&dwinv, sizeof(double) * Np * GPK_TILE));
  CHECK_HIP(hipMalloc((void**)&dA, sizeof(double) * N * P));
  CHECK_HIP(hipMalloc((void**)&dAT, sizeof(double) * N * P));
  CHECK_HIP(hipMemset(dK, 0xFF, sizeof(double) * nK));
  CHECK_HIP(hipMemset(dW, 0xFF, sizeof(double) * nK));
  CHECK_HIP(hipMemset(dtr, 0xFF, sizeof(double) * ntr));

  /* ---- fit: K = k(X, X) + (noise + alpha) I, L, W = L^-1, alpha = W^T (W Yn) - once (N x P), once per output (N x 1) -------- */
  int info = -1;
  CHECK_GPK(gpk_gram(h, GPK_F64, dX, N, D, ls, sf2, noise + alpha_j, dK, Np));
  CHECK_GPK(gpk_potrf(h, dK, Np, Np, dwinv, &info));
  EXPECT(info == 0, "potrf info %d", info);
  CHECK_GPK(gpk_trtri(h, dK, Np, Np, dwinv, dW, Np, dtr));
  CHECK_GPK(gpk_potrs_inv(h, dW, Np, Np, dYn, N, P, dA));
  for (int b = 0; b < P; ++b) CHECK_GPK(gpk_potrs_inv(h, dW, Np, Np, dYnT + (long)b * N, N, 1, dAT + (long)b * N));
  CHECK_GPK(gpk_synchronize(h));

  const size_t nT = (size_t)(H + 1) * R * P, nS = nT * P, nM = (size_t)H * R * P, nJ = nM * D, nAll = nT + nS + 2 * nM + nJ;
  double* out = (double*)malloc(sizeof(double) * 2 * nAll);
  double* again = (double*)malloc(sizeof(double) * nAll);
  for (size_t i = 0; i < 2 * nAll; ++i) out[i] = NAN;
  double *t1 = out, *s1 = t1 + nT, *m1 = s1 + nS, *v1 = m1 + nM, *j1 = v1 + nM;
  double *t2 = out + nAll, *s2 = t2 + nT, *m2 = s2 + nS, *v2 = m2 + nM, *j2 = v2 + nM;
  double *ta = again, *sa = ta + nT, *ma = sa + nS, *va = ma + nM, *ja = va + nM;
  const double kss = sf2 + noise;

  /* ---- gpk_propagate_host: the call, the same bits again, NULL stage outputs ---------------------------------------------- */
#define SINGLE(R_, H_, x0_, xr_, U_, ur_, lin_, S0_, sr_, Q_, t_, s_, m_, v_, j_) \
  gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0_, xr_, U_, ur_, lin_, S0_, sr_, Q_, R_, H_, t_, s_, m_, v_, j_)
  CHECK_GPK(SINGLE(R, H, x0, R, U, R, lin, S0, 1, Q, t1, s1, m1, v1, j1));
  for (size_t i = 0; i < nAll; ++i) { EXPECT(isfinite(out[i]), "single: out[%zu] is not finite", i); again[i] = NAN; }
  CHECK_GPK(SINGLE(R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, ma, va, ja));
  EXPECT(!memcmp(again, out, sizeof(double) * nAll), "gpk_propagate_host: two calls differ");
  for (size_t i = 0; i < nT + nS; ++i) again[i] = NAN;
  CHECK_GPK(SINGLE(R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL));
  EXPECT(!memcmp(again, out, sizeof(double) * (nT + nS)), "gpk_propagate_host: NULL stage outputs changed traj or Sigma");
  EXPECT(!memcmp(t1, x0, sizeof(double) * R * P), "stage 0 of the trajectory is not x0");
  for (long k = 0; k < (long)(H + 1) * R; ++k)
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < i; ++j)
        EXPECT(!memcmp(s1 + k * P * P + i * P + j, s1 + k * P * P + j * P + i, sizeof(double)), "Sigma block %ld is not symmetric", k);
  /* one start and one control sequence for every rollout: rollout 0 keeps its bits */
  CHECK_GPK(SINGLE(R, H, x0, 1, U, 1, lin, NULL, 1, NULL, ta, sa, NULL, NULL, NULL));
  for (int r = 0; r < R; ++r) EXPECT(!memcmp(ta + (long)r * P, x0, sizeof(double) * P), "broadcast start, rollout %d", r);
  for (int r = 1; r < R; ++r)
    for (int k = 0; k <= H; ++k)
      EXPECT(!memcmp(ta + ((long)k * R + r) * P, ta + (long)k * R * P, sizeof(double) * P), "broadcast rollouts differ at stage %d", k);

  /* ---- gpk_propagate_host_multi: B = P models on coord 0 .. B - 1 behind the input scaler, noise through var_includes_noise --- */
  const int B = P;
  const double *Xs[8], *As[8], *Ws[8];
  double lsB[8 * 16], sf2B[8], kssB[8], noiseB[8];
  int coord[8];
  for (int b = 0; b < B; ++b) {
    Xs[b] = dX; As[b] = dAT + (long)b * N; Ws[b] = dW;
    memcpy(lsB + b * D, ls, sizeof(double) * D);
    sf2B[b] = sf2; kssB[b] = sf2; noiseB[b] = noise; coord[b] = b;
  }
#define MULTI(B_, nx_, coord_, ish_, isc_, R_, H_, x0_, xr_, U_, ur_, S0_, sr_, t_, s_, m_, v_, j_) \
  gpk_propagate_host_multi(h, B_, Xs, As, N, D, lsB, sf2B, ym, ys, Ws, Np, Np, kssB, 0.0, 1, noiseB, nx_, coord_, ish_, isc_, x0_, xr_, U_, ur_, lin, S0_, sr_, Q, R_, H_, t_, s_, m_, v_, j_)
  CHECK_GPK(MULTI(B, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, t2, s2, m2, v2, j2));
  for (size_t i = nAll; i < 2 * nAll; ++i) EXPECT(isfinite(out[i]), "multi: out[%zu] is not finite", i);
  for (size_t i = 0; i < nAll; ++i) again[i] = NAN;
  CHECK_GPK(MULTI(B, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, ma, va, ja));
  EXPECT(!memcmp(again, out + nAll, sizeof(double) * nAll), "gpk_propagate_host_multi: two calls differ");
  for (size_t i = 0; i < nT + nS; ++i) again[i] = NAN;
  CHECK_GPK(MULTI(B, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL));
  EXPECT(!memcmp(again, out + nAll, sizeof(double) * (nT + nS)), "gpk_propagate_host_multi: NULL stage outputs changed traj or Sigma");

  /* ---- bad arguments: statuses, never a fault ------------------------------------------------------------------------------ */
  BAD(gpk_propagate_host(NULL, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "null handle");
  BAD(SINGLE(0, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "R = 0");
  BAD(SINGLE(33, H, x0, 1, U, 1, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "R = 33");
  EXPECT(strstr(gpk_last_error(h), "R must be in [1, 32]") != NULL, "message: %s", gpk_last_error(h));
  BAD(SINGLE(R, 0, x0, R, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "H = 0");
  BAD(SINGLE(R, 257, x0, R, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "H = 257");
  EXPECT(strstr(gpk_last_error(h), "H must be in [1, 256]") != NULL, "message: %s", gpk_last_error(h));
  BAD(SINGLE(R, H, NULL, R, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "null x0");
  BAD(SINGLE(R, H, x0, R, NULL, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "null U with D > P");
  BAD(SINGLE(R, H, x0, R, U, R, NULL, S0, 1, Q, ta, sa, NULL, NULL, NULL), "null lin");
  BAD(SINGLE(R, H, x0, R, U, R, lin, S0, 1, Q, NULL, sa, NULL, NULL, NULL), "null traj");
  BAD(SINGLE(R, H, x0, R, U, R, lin, S0, 1, Q, ta, NULL, NULL, NULL, NULL), "null Sigma");
  if (R > 2) {
    BAD(SINGLE(R, H, x0, 2, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "x0 with 2 rows");
    BAD(SINGLE(R, H, x0, R, U, 2, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "U with 2 rows");
    BAD(SINGLE(R, H, x0, R, U, R, lin, S0, 2, Q, ta, sa, NULL, NULL, NULL), "Sigma0 with 2 rows");
  }
  BAD(gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, NULL, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "null W");
  BAD(gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np + 128, Np + 128, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "Np != gpk_padded(N)");
  BAD(gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np - 1, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "ldw < Np");
  BAD(gpk_propagate_host(h, dX, dA, N, P - 1, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "P > D");
  BAD(gpk_propagate_host(h, dX, dA, N, 17, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "D = 17");
  BAD(gpk_propagate_host(h, dX, dA, 16385, D, P, ls, sf2, ym, ys, dW, 16512, 16512, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "gpk_padded(N) > 16384");
  BAD(gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 1, NAN, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "NaN noise");
  {
    /* the model's own host arrays: NaN or infinity, or a length-scale that is not positive, is refused before any launch */
    double bls[16], bym[16], bys[16];
    memcpy(bls, ls, sizeof(double) * D); memcpy(bym, ym, sizeof(double) * P); memcpy(bys, ys, sizeof(double) * P);
    bls[D - 1] = NAN; bym[0] = INFINITY; bys[P - 1] = NAN;
    BAD(gpk_propagate_host(h, dX, dA, N, D, P, bls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "NaN in ls");
    BAD(gpk_propagate_host(h, dX, dA, N, D, P, ls, NAN, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "NaN sf2");
    BAD(gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, bym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "infinity in y_mean");
    BAD(gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, ym, bys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "NaN in y_std");
    EXPECT(strstr(gpk_last_error(h), "ls, sf2, y_mean and y_std") != NULL, "message: %s", gpk_last_error(h));
    bls[D - 1] = -1.0;
    BAD(gpk_propagate_host(h, dX, dA, N, D, P, bls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "negative length-scale");
    EXPECT(strstr(gpk_last_error(h), "positive") != NULL, "message: %s", gpk_last_error(h));
  }
  {
    double* bad = (double*)malloc(sizeof(double) * ((long)R * P + (long)R * H * nu + P * D + 2 * P * P));
    double *bx = bad, *bu = bx + (long)R * P, *bl = bu + (long)R * H * nu, *bs = bl + P * D, *bq = bs + P * P;
    memcpy(bx, x0, sizeof(double) * R * P); memcpy(bu, U, sizeof(double) * R * H * nu); memcpy(bl, lin, sizeof(double) * P * D);
    memcpy(bs, S0, sizeof(double) * P * P); memcpy(bq, Q, sizeof(double) * P * P);
    bx[(long)R * P - 1] = NAN; bu[(long)R * H * nu - 1] = INFINITY; bl[0] = -INFINITY; bs[1] = NAN; bq[P * P - 1] = INFINITY;
    BAD(SINGLE(R, H, bx, R, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "NaN in x0");
    BAD(SINGLE(R, H, x0, R, bu, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "infinity in U");
    BAD(SINGLE(R, H, x0, R, U, R, bl, S0, 1, Q, ta, sa, NULL, NULL, NULL), "infinity in lin");
    BAD(SINGLE(R, H, x0, R, U, R, lin, bs, 1, Q, ta, sa, NULL, NULL, NULL), "NaN in Sigma0");
    BAD(SINGLE(R, H, x0, R, U, R, lin, S0, 1, bq, ta, sa, NULL, NULL, NULL), "infinity in Q");
    EXPECT(strstr(gpk_last_error(h), "NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    free(bad);
  }
  {
    int twice[8] = {0, 0, 2, 3, 4, 5, 6, 7}, far[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    far[B - 1] = P;
    double zero_scale[16], nan_shift[16];
    memcpy(zero_scale, isc, sizeof(double) * D); memcpy(nan_shift, ish, sizeof(double) * D);
    zero_scale[D - 1] = 0.0; nan_shift[0] = NAN;
    BAD(MULTI(0, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "B = 0");
    BAD(MULTI(9, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "B = 9");
    BAD(MULTI(B, P, twice, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "coord repeated");
    EXPECT(strstr(gpk_last_error(h), "distinct") != NULL, "message: %s", gpk_last_error(h));
    BAD(MULTI(B, P, far, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "coord = nx");
    BAD(MULTI(B, P, NULL, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "null coord");
    BAD(MULTI(B, B - 1, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "nx < B");
    BAD(MULTI(B, D + 1, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "nx > D");
    BAD(MULTI(B, P, coord, ish, NULL, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "in_shift without in_scale");
    BAD(MULTI(B, P, coord, ish, zero_scale, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "in_scale = 0");
    EXPECT(strstr(gpk_last_error(h), "non-zero") != NULL, "message: %s", gpk_last_error(h));
    BAD(MULTI(B, P, coord, nan_shift, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "NaN in in_shift");
    BAD(MULTI(B, P, coord, ish, isc, 33, H, x0, 1, U, 1, S0, 1, ta, sa, NULL, NULL, NULL), "R = 33");
    BAD(MULTI(B, P, coord, ish, isc, R, 257, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "H = 257");
    Ws[0] = NULL;
    BAD(MULTI(B, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "null W of model 0");
    Ws[0] = dW;
    lsB[(B - 1) * D] = NAN;
    BAD(MULTI(B, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "NaN in the last model's ls");
    lsB[(B - 1) * D] = ls[0];
    sf2B[B - 1] = INFINITY;
    BAD(MULTI(B, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "infinite sf2 of the last model");
    EXPECT(strstr(gpk_last_error(h), "ls, sf2, y_mean and y_std") != NULL, "message: %s", gpk_last_error(h));
    sf2B[B - 1] = sf2;
  }
  CHECK_GPK(gpk_batch_begin(h, 2));
  BAD(SINGLE(R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL), "batched mode");
  BAD(MULTI(B, P, coord, ish, isc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "batched mode");
  CHECK_GPK(gpk_batch_end(h));
  /* the refusals left the handle serving: the same bits once more */
  CHECK_GPK(SINGLE(R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, ma, va, ja));
  EXPECT(!memcmp(again, out, sizeof(double) * nAll), "gpk_propagate_host changed under the refused calls");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), 2 * nAll, f) != 2 * nAll) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  hipFree(dX); hipFree(dYn); hipFree(dYnT); hipFree(dK); hipFree(dW); hipFree(dtr); hipFree(dwinv); hipFree(dA); hipFree(dAT);
  gpk_destroy(h);
  free(again); free(out); free(buf);
  printf("propagate from C: OK\n");
  return 0;
}
