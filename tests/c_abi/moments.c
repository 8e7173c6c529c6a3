/* Exact moment matching (K11) from a plain C caller - no Python, no torch: the fit building blocks (gpk_gram -> gpk_potrf ->
 * gpk_trtri -> gpk_potrs_inv, then gpk_wtw for K^-1) on hipMalloc'd buffers, then gpk_moments_host and gpk_propagate_mm_host on the
 * model with P outputs, and gpk_moments_host_multi and gpk_propagate_mm_host_multi on the same outputs as B = P single-output
 * models behind an input scaler.
 * The pytest wrapper (tests/test_gpu_moments_c_abi.py) writes the problem as one flat file of doubles, argv[1] (the layout of
 * tests/c_abi/propagate.c):
 *   [N, D, P, R, H, sf2, noise, alpha]  ls (D)  y_mean (P)  y_std (P)  X (N x D)  Yn (N x P)  YnT (P x N)  x0 (R x P)
 *   U (R x H x (D - P))  lin (P x D)  Sigma0 (P x P)  Q (P x P)  in_shift (D)  in_scale (D)
 * and compares what this program writes to argv[2] with the dense NumPy form, for the single model and then for the batch:
 *   moments at the R Gaussian queries ([x0[r], U[r][0]], Sigma0):  mean (R x P)  cov (R x P x P)  xcov (R x P x D)
 *   the horizon:  traj ((H + 1) x R x P)  Sigma ((H + 1) x R x P x P)  mean (H x R x P)  cov (H x R x P x P)  xcov (H x R x P x D)
 * The program itself checks that repeated calls repeat their bits, that NULL stage outputs change nothing, that cov and Sigma are
 * symmetric bit for bit, and that every bad-argument status comes back with the output arrays untouched.
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
/* a refusal: the status, and the canary-filled outputs `ta` (nAll doubles) untouched */
#define BAD(call, what) do { EXPECT((call) == GPK_BAD_ARG, what); for (size_t i_ = 0; i_ < nAll; ++i_) EXPECT(!memcmp(again + i_, &canary, sizeof(double)), "%s: output %zu written", what, i_); } while (0)

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
  double *dK, *dW, *dKi, *dtr, *dwinv, *dA, *dAT;
  const size_t nK = (size_t)Np * Np, ntr = (size_t)(Np / 2 + 128) * (Np / 2 + 128);
  CHECK_HIP(hipMalloc((void**)&dK, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dW, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dKi, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dtr, sizeof(double) * ntr));
  CHECK_HIP(hipMalloc((void**)&dwinv, sizeof(double) * Np * GPK_TILE));
  CHECK_HIP(hipMalloc((void**)&dA, sizeof(double) * N * P));
  CHECK_HIP(hipMalloc((void**)&dAT, sizeof(double) * N * P));
  CHECK_HIP(hipMemset(dK, 0xFF, sizeof(double) * nK));
  CHECK_HIP(hipMemset(dW, 0xFF, sizeof(double) * nK));
  CHECK_HIP(hipMemset(dKi, 0xFF, sizeof(double) * nK));      /* NaN above the lower tiles: the entries must never read them */
  CHECK_HIP(hipMemset(dtr, 0xFF, sizeof(double) * ntr));

  /* ---- fit: K = k(X, X) + (noise + alpha) I, L, W = L^-1, alpha = W^T (W Yn), K^-1 = W^T W ------------------------------------ */
  int info = -1;
  CHECK_GPK(gpk_gram(h, GPK_F64, dX, N, D, ls, sf2, noise + alpha_j, dK, Np));
  CHECK_GPK(gpk_potrf(h, dK, Np, Np, dwinv, &info));
  EXPECT(info == 0, "potrf info %d", info);
  CHECK_GPK(gpk_trtri(h, dK, Np, Np, dwinv, dW, Np, dtr));
  CHECK_GPK(gpk_potrs_inv(h, dW, Np, Np, dYn, N, P, dA));
  for (int b = 0; b < P; ++b) CHECK_GPK(gpk_potrs_inv(h, dW, Np, Np, dYnT + (long)b * N, N, 1, dAT + (long)b * N));
  CHECK_GPK(gpk_wtw(h, dW, Np, Np, dKi, Np));
  CHECK_GPK(gpk_synchronize(h));

  /* the R Gaussian queries of the moments calls: [x0[r], U[r][0]] with covariance Sigma0 */
  double* Xq = (double*)malloc(sizeof(double) * R * D);
  double* Sq = (double*)malloc(sizeof(double) * R * P * P);
  for (int r = 0; r < R; ++r) {
    memcpy(Xq + (long)r * D, x0 + (long)r * P, sizeof(double) * P);
    memcpy(Xq + (long)r * D + P, U + (long)r * H * nu, sizeof(double) * nu);
    memcpy(Sq + (long)r * P * P, S0, sizeof(double) * P * P);
  }
  const size_t qM = (size_t)R * P, qC = qM * P, qX = qM * D, nQ = qM + qC + qX;
  const size_t nT = (size_t)(H + 1) * R * P, nS = nT * P, nM = (size_t)H * R * P, nC = nM * P, nJ = nM * D;
  const size_t nAll = nQ + nT + nS + nM + nC + nJ;
  double* out = (double*)malloc(sizeof(double) * 2 * nAll);
  double* again = (double*)malloc(sizeof(double) * nAll);
  double canary;
  memset(&canary, 0xA5, sizeof(double));
  for (size_t i = 0; i < 2 * nAll; ++i) out[i] = NAN;
  const double kss = sf2;
#define BLOCKS(p, qm, qc, qx, t, s, m, c, x) double *qm = (p), *qc = qm + qM, *qx = qc + qC, *t = qx + qX, *s = t + nT, *m = s + nS, *c = m + nM, *x = c + nC
  BLOCKS(out, qm1, qc1, qx1, t1, s1, m1, c1, x1);
  BLOCKS(out + nAll, qm2, qc2, qx2, t2, s2, m2, c2, x2);
  BLOCKS(again, qma, qca, qxa, ta, sa, ma, ca, xa);

  /* ---- the single model ------------------------------------------------------------------------------------------------------- */
#define MOM(Ki_, Np_, ldk_, nx_, Xq_, Sq_, M_, m_, c_, x_) \
  gpk_moments_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, Ki_, Np_, ldk_, kss, 0.0, 0, 0.0, nx_, Xq_, Sq_, M_, m_, c_, x_)
#define CHAIN(Ki_, ldk_, R_, H_, x0_, xr_, U_, ur_, lin_, S0_, sr_, Q_, t_, s_, m_, c_, x_) \
  gpk_propagate_mm_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, Ki_, Np, ldk_, kss, 0.0, 0, 0.0, x0_, xr_, U_, ur_, lin_, S0_, sr_, Q_, R_, H_, t_, s_, m_, c_, x_)
  CHECK_GPK(MOM(dKi, Np, Np, P, Xq, Sq, R, qm1, qc1, qx1));
  CHECK_GPK(CHAIN(dKi, Np, R, H, x0, R, U, R, lin, S0, 1, Q, t1, s1, m1, c1, x1));
  for (size_t i = 0; i < nAll; ++i) { EXPECT(isfinite(out[i]), "single: out[%zu] is not finite", i); again[i] = NAN; }
  CHECK_GPK(MOM(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa));
  CHECK_GPK(CHAIN(dKi, Np, R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, ma, ca, xa));
  EXPECT(!memcmp(again, out, sizeof(double) * nAll), "single: two calls differ");
  for (size_t i = 0; i < nT + nS; ++i) ta[i] = NAN;
  CHECK_GPK(CHAIN(dKi, Np, R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, NULL, NULL, NULL));
  EXPECT(!memcmp(ta, t1, sizeof(double) * (nT + nS)), "gpk_propagate_mm_host: NULL stage outputs changed traj or Sigma");
  EXPECT(!memcmp(t1, x0, sizeof(double) * R * P), "stage 0 of the trajectory is not x0");
  EXPECT(!memcmp(m1, qm1, sizeof(double) * qM) && !memcmp(c1, qc1, sizeof(double) * qC) && !memcmp(x1, qx1, sizeof(double) * qX),
         "stage 0 of the chain does not have the bits of gpk_moments_host at its queries");
  for (long k = 0; k < (long)(H + 1) * R; ++k)
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < i; ++j)
        EXPECT(!memcmp(s1 + k * P * P + i * P + j, s1 + k * P * P + j * P + i, sizeof(double)), "Sigma block %ld is not symmetric", k);
  for (long k = 0; k < (long)H * R; ++k)
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < i; ++j)
        EXPECT(!memcmp(c1 + k * P * P + i * P + j, c1 + k * P * P + j * P + i, sizeof(double)), "cov block %ld is not symmetric", k);

  /* ---- the batch: B = P models on coord 0 .. B - 1 behind the input scaler, the noise level through var_includes_noise ---------- */
  const int B = P;
  const double *Xs[8], *As[8], *Ks[8];
  double lsB[8 * 16], sf2B[8], kssB[8], noiseB[8];
  int coord[8];
  for (int b = 0; b < B; ++b) {
    Xs[b] = dX; As[b] = dAT + (long)b * N; Ks[b] = dKi;
    memcpy(lsB + b * D, ls, sizeof(double) * D);
    sf2B[b] = sf2; kssB[b] = sf2; noiseB[b] = noise; coord[b] = b;
  }
#define MMOM(B_, nx_, ish_, isc_, M_, m_, c_, x_) \
  gpk_moments_host_multi(h, B_, Xs, As, N, D, lsB, sf2B, ym, ys, Ks, Np, Np, kssB, 0.0, 1, noiseB, nx_, ish_, isc_, Xq, Sq, M_, m_, c_, x_)
#define MCHAIN(B_, nx_, coord_, ish_, isc_, R_, H_, S0_, t_, s_, m_, c_, x_) \
  gpk_propagate_mm_host_multi(h, B_, Xs, As, N, D, lsB, sf2B, ym, ys, Ks, Np, Np, kssB, 0.0, 1, noiseB, nx_, coord_, ish_, isc_, x0, R, U, R, lin, S0_, 1, Q, R_, H_, t_, s_, m_, c_, x_)
  CHECK_GPK(MMOM(B, P, ish, isc, R, qm2, qc2, qx2));
  CHECK_GPK(MCHAIN(B, P, coord, ish, isc, R, H, S0, t2, s2, m2, c2, x2));
  for (size_t i = nAll; i < 2 * nAll; ++i) EXPECT(isfinite(out[i]), "multi: out[%zu] is not finite", i);
  for (size_t i = 0; i < nAll; ++i) again[i] = NAN;
  CHECK_GPK(MMOM(B, P, ish, isc, R, qma, qca, qxa));
  CHECK_GPK(MCHAIN(B, P, coord, ish, isc, R, H, S0, ta, sa, ma, ca, xa));
  EXPECT(!memcmp(again, out + nAll, sizeof(double) * nAll), "multi: two calls differ");
  EXPECT(!memcmp(m2, qm2, sizeof(double) * qM) && !memcmp(c2, qc2, sizeof(double) * qC) && !memcmp(x2, qx2, sizeof(double) * qX),
         "stage 0 of the batch chain does not have the bits of gpk_moments_host_multi at its queries");

  /* ---- bad arguments: statuses before any launch, the outputs untouched ---------------------------------------------------------- */
  for (size_t i = 0; i < nAll; ++i) memcpy(again + i, &canary, sizeof(double));
  BAD(gpk_moments_host(NULL, dX, dA, N, D, P, ls, sf2, ym, ys, dKi, Np, Np, kss, 0.0, 0, 0.0, P, Xq, Sq, R, qma, qca, qxa), "null handle");
  BAD(MOM(NULL, Np, Np, P, Xq, Sq, R, qma, qca, qxa), "moments: null K^-1");
  EXPECT(strstr(gpk_last_error(h), "K^-1") != NULL, "message: %s", gpk_last_error(h));
  BAD(MOM(dKi, Np, Np - 1, P, Xq, Sq, R, qma, qca, qxa), "moments: ldk < Np");
  EXPECT(strstr(gpk_last_error(h), "ldk >= Np") != NULL, "message: %s", gpk_last_error(h));
  BAD(MOM(dKi, Np + 128, Np + 128, P, Xq, Sq, R, qma, qca, qxa), "moments: Np != gpk_padded(N)");
  BAD(MOM(dKi, Np, Np, P, Xq, Sq, 0, qma, qca, qxa), "moments: M = 0");
  BAD(MOM(dKi, Np, Np, P, Xq, Sq, 33, qma, qca, qxa), "moments: M = 33");
  EXPECT(strstr(gpk_last_error(h), "M must be in [1, 32]") != NULL, "message: %s", gpk_last_error(h));
  BAD(MOM(dKi, Np, Np, D + 1, Xq, Sq, R, qma, qca, qxa), "moments: nx > D");
  BAD(MOM(dKi, Np, Np, P, NULL, Sq, R, qma, qca, qxa), "moments: null queries");
  BAD(MOM(dKi, Np, Np, P, Xq, Sq, R, NULL, qca, qxa), "moments: null mean");
  BAD(CHAIN(NULL, Np, R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: null K^-1");
  BAD(CHAIN(dKi, Np - 1, R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: ldk < Np");
  BAD(CHAIN(dKi, Np, 33, H, x0, 1, U, 1, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: R = 33");
  EXPECT(strstr(gpk_last_error(h), "R must be in [1, 32]") != NULL, "message: %s", gpk_last_error(h));
  BAD(CHAIN(dKi, Np, R, 0, x0, R, U, R, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: H = 0");
  BAD(CHAIN(dKi, Np, R, 257, x0, R, U, R, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: H = 257");
  BAD(CHAIN(dKi, Np, R, H, NULL, R, U, R, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: null x0");
  BAD(CHAIN(dKi, Np, R, H, x0, R, NULL, R, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: null U with D > P");
  BAD(CHAIN(dKi, Np, R, H, x0, R, U, R, lin, S0, 1, Q, NULL, sa, ma, ca, xa), "chain: null traj");
  if (R > 2) BAD(CHAIN(dKi, Np, R, H, x0, 2, U, R, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: x0 with 2 rows");
  {
    double bs[64], bq[16 * 16], bls[16];
    memcpy(bs, S0, sizeof(double) * P * P); bs[P * P - 1] = INFINITY;
    BAD(CHAIN(dKi, Np, R, H, x0, R, U, R, lin, bs, 1, Q, ta, sa, ma, ca, xa), "chain: infinity in Sigma0");
    EXPECT(strstr(gpk_last_error(h), "Sigma0 must not contain NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    bs[P * P - 1] = S0[P * P - 1]; bs[P] = NAN;      /* (entry (1, 0): in the lower triangle) */
    BAD(CHAIN(dKi, Np, R, H, x0, R, U, R, lin, bs, 1, Q, ta, sa, ma, ca, xa), "chain: NaN in Sigma0");
    double* bsq = (double*)malloc(sizeof(double) * R * P * P);
    memcpy(bsq, Sq, sizeof(double) * R * P * P); bsq[(long)R * P * P - 1] = NAN;
    BAD(MOM(dKi, Np, Np, P, Xq, bsq, R, qma, qca, qxa), "moments: NaN in a covariance");
    EXPECT(strstr(gpk_last_error(h), "covariances must not contain NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    free(bsq);
    memcpy(bq, Xq, sizeof(double) * D); bq[D - 1] = INFINITY;
    BAD(MOM(dKi, Np, Np, P, bq, Sq, 1, qma, qca, qxa), "moments: infinity in a query");
    memcpy(bls, ls, sizeof(double) * D); bls[0] = -1.0;
    BAD(gpk_moments_host(h, dX, dA, N, D, P, bls, sf2, ym, ys, dKi, Np, Np, kss, 0.0, 0, 0.0, P, Xq, Sq, R, qma, qca, qxa), "negative length-scale");
    BAD(gpk_moments_host(h, dX, dA, N, D, P, ls, NAN, ym, ys, dKi, Np, Np, kss, 0.0, 0, 0.0, P, Xq, Sq, R, qma, qca, qxa), "NaN sf2");
  }
  {
    int twice[8] = {0, 0, 2, 3, 4, 5, 6, 7};
    double zero_scale[16];
    memcpy(zero_scale, isc, sizeof(double) * D); zero_scale[D - 1] = 0.0;
    BAD(MMOM(0, P, ish, isc, R, qma, qca, qxa), "multi moments: B = 0");
    BAD(MMOM(9, P, ish, isc, R, qma, qca, qxa), "multi moments: B = 9");
    BAD(MMOM(B, P, ish, NULL, R, qma, qca, qxa), "multi moments: in_shift without in_scale");
    BAD(MMOM(B, P, ish, zero_scale, R, qma, qca, qxa), "multi moments: in_scale = 0");
    BAD(MCHAIN(B, P, twice, ish, isc, R, H, S0, ta, sa, ma, ca, xa), "multi chain: coord repeated");
    EXPECT(strstr(gpk_last_error(h), "distinct") != NULL, "message: %s", gpk_last_error(h));
    BAD(MCHAIN(B, P, NULL, ish, isc, R, H, S0, ta, sa, ma, ca, xa), "multi chain: null coord");
    BAD(MCHAIN(B, B - 1, coord, ish, isc, R, H, S0, ta, sa, ma, ca, xa), "multi chain: nx < B");
    Ks[B - 1] = NULL;
    BAD(MMOM(B, P, ish, isc, R, qma, qca, qxa), "multi moments: null K^-1 of the last model");
    BAD(MCHAIN(B, P, coord, ish, isc, R, H, S0, ta, sa, ma, ca, xa), "multi chain: null K^-1 of the last model");
    EXPECT(strstr(gpk_last_error(h), "K^-1") != NULL, "message: %s", gpk_last_error(h));
    Ks[B - 1] = dKi;
  }
  CHECK_GPK(gpk_batch_begin(h, 2));
  BAD(MOM(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa), "moments: batched mode");
  BAD(CHAIN(dKi, Np, R, H, x0, R, U, R, lin, S0, 1, Q, ta, sa, ma, ca, xa), "chain: batched mode");
  CHECK_GPK(gpk_batch_end(h));
  /* after all the refusals the entries still serve */
  CHECK_GPK(MOM(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa));
  EXPECT(!memcmp(qma, qm1, sizeof(double) * qM), "moments after the refusals: the bits changed");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), 2 * nAll, f) != 2 * nAll) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  gpk_destroy(h);
  printf("moments from C: OK\n");
  return 0;
}
