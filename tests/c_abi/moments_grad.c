/* The gradient through exact moment matching (K11) from a plain C caller - no Python, no torch: the fit building blocks and gpk_wtw
 * on hipMalloc'd buffers (as tests/c_abi/moments.c), then gpk_moments_vjp_host and gpk_propagate_mm_grad_host on the model with P
 * outputs, and gpk_moments_vjp_host_multi and gpk_propagate_mm_grad_host_multi on the same outputs as B = P single-output models
 * behind an input scaler.
 * The pytest wrapper (tests/test_gpu_moments_grad_c_abi.py) writes the problem as one flat file of doubles, argv[1]:
 *   [N, D, P, R, H, sf2, noise, alpha]  ls (D)  y_mean (P)  y_std (P)  X (N x D)  Yn (N x P)  YnT (P x N)  x0 (R x P)
 *   U (R x H x (D - P))  lin (P x D)  Sigma0 (P x P)  Q (P x P)  in_shift (D)  in_scale (D)
 *   gmean (R x P)  gcov (R x P x P)  gxcov (R x P x D)  gx ((H + 1) x R x P)  gS ((H + 1) x R x P x P)
 * and compares what this program writes to argv[2] with the dense NumPy adjoint, for the single model and then for the batch:
 *   at the R Gaussian queries ([x0[r], U[r][0]], Sigma0):  mean (R x P)  cov (R x P x P)  xcov (R x P x D)  dXq (R x D)  dSq (R x P x P)
 *   the horizon:  traj ((H + 1) x R x P)  Sigma ((H + 1) x R x P x P)  dU (R x H x nu)  dx0 (R x P)  dSigma0 (R x P x P)
 * The program itself checks that mean, cov, xcov, traj and Sigma have the bits of the forward entries, that repeated calls repeat
 * their bits, that NULL seeds are seeds of zeros, that dSq and dSigma0 are symmetric bit for bit, and that every bad-argument status
 * comes back with the output arrays untouched.
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
/* a refusal: the status, and the canary-filled outputs `again` (nAll doubles) untouched */
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
  const double *gm = isc + D, *gc = gm + (long)R * P, *gxc = gc + (long)R * P * P, *gx = gxc + (long)R * P * D;
  const double* gS = gx + (long)(H + 1) * R * P;
  EXPECT((gS + (long)(H + 1) * R * P * P - buf) * (long)sizeof(double) == bytes && nu >= 1 && P >= 2 && P <= 8, "file layout: %ld bytes", bytes);

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

  /* the R Gaussian queries of the query entries: [x0[r], U[r][0]] with covariance Sigma0 */
  double* Xq = (double*)malloc(sizeof(double) * R * D);
  double* Sq = (double*)malloc(sizeof(double) * R * P * P);
  for (int r = 0; r < R; ++r) {
    memcpy(Xq + (long)r * D, x0 + (long)r * P, sizeof(double) * P);
    memcpy(Xq + (long)r * D + P, U + (long)r * H * nu, sizeof(double) * nu);
    memcpy(Sq + (long)r * P * P, S0, sizeof(double) * P * P);
  }
  const size_t qM = (size_t)R * P, qC = qM * P, qX = qM * D, qD = (size_t)R * D, qS = qC;
  const size_t nT = (size_t)(H + 1) * R * P, nS = nT * P, nU = (size_t)R * H * nu, nx0 = qM, nS0 = qC;
  const size_t nAll = qM + qC + qX + qD + qS + nT + nS + nU + nx0 + nS0;
  double* out = (double*)malloc(sizeof(double) * 2 * nAll);
  double* again = (double*)malloc(sizeof(double) * nAll);
  double* fwd = (double*)malloc(sizeof(double) * nAll);
  double canary;
  memset(&canary, 0xA5, sizeof(double));
  for (size_t i = 0; i < 2 * nAll; ++i) out[i] = NAN;
  const double kss = sf2;
#define BLOCKS(p, qm, qc, qx, qd, qs, t, s, du, dx, ds) \
  double *qm = (p), *qc = qm + qM, *qx = qc + qC, *qd = qx + qX, *qs = qd + qD, *t = qs + qS, *s = t + nT, *du = s + nS, *dx = du + nU, *ds = dx + nx0
  BLOCKS(out, qm1, qc1, qx1, qd1, qs1, t1, s1, du1, dx1, ds1);
  BLOCKS(out + nAll, qm2, qc2, qx2, qd2, qs2, t2, s2, du2, dx2, ds2);
  BLOCKS(again, qma, qca, qxa, qda, qsa, ta, sa, dua, dxa, dsa);
  BLOCKS(fwd, qmf, qcf, qxf, qdf, qsf, tf, sf, duf, dxf, dsf);
  (void)qdf; (void)qsf; (void)duf; (void)dxf; (void)dsf;

  /* ---- the single model ------------------------------------------------------------------------------------------------------- */
#define VJP(Ki_, Np_, ldk_, nx_, Xq_, Sq_, M_, m_, c_, x_, gm_, gc_, gx_, d_, s_) \
  gpk_moments_vjp_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, Ki_, Np_, ldk_, kss, 0.0, 0, 0.0, nx_, Xq_, Sq_, M_, m_, c_, x_, gm_, gc_, gx_, d_, s_)
#define GRAD(Ki_, ldk_, R_, H_, x0_, xr_, U_, ur_, S0_, t_, s_, gx_, gS_, du_, dx_, ds_) \
  gpk_propagate_mm_grad_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, Ki_, Np, ldk_, kss, 0.0, 0, 0.0, x0_, xr_, U_, ur_, lin, S0_, 1, Q, R_, H_, t_, s_, NULL, NULL, NULL, gx_, gS_, du_, dx_, ds_)
  CHECK_GPK(VJP(dKi, Np, Np, P, Xq, Sq, R, qm1, qc1, qx1, gm, gc, gxc, qd1, qs1));
  CHECK_GPK(GRAD(dKi, Np, R, H, x0, R, U, R, S0, t1, s1, gx, gS, du1, dx1, ds1));
  for (size_t i = 0; i < nAll; ++i) { EXPECT(isfinite(out[i]), "single: out[%zu] is not finite", i); again[i] = NAN; }
  CHECK_GPK(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa));
  CHECK_GPK(GRAD(dKi, Np, R, H, x0, R, U, R, S0, ta, sa, gx, gS, dua, dxa, dsa));
  EXPECT(!memcmp(again, out, sizeof(double) * nAll), "single: two calls differ");
  CHECK_GPK(gpk_moments_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dKi, Np, Np, kss, 0.0, 0, 0.0, P, Xq, Sq, R, qmf, qcf, qxf));
  CHECK_GPK(gpk_propagate_mm_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dKi, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H,
                                  tf, sf, NULL, NULL, NULL));
  EXPECT(!memcmp(qm1, qmf, sizeof(double) * (qM + qC + qX)), "gpk_moments_vjp_host: mean, cov, xcov do not have gpk_moments_host's bits");
  EXPECT(!memcmp(t1, tf, sizeof(double) * (nT + nS)), "gpk_propagate_mm_grad_host: traj, Sigma do not have gpk_propagate_mm_host's bits");
  for (long k = 0; k < R; ++k)
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < i; ++j) {
        EXPECT(!memcmp(qs1 + k * P * P + i * P + j, qs1 + k * P * P + j * P + i, sizeof(double)), "dSq block %ld is not symmetric", k);
        EXPECT(!memcmp(ds1 + k * P * P + i * P + j, ds1 + k * P * P + j * P + i, sizeof(double)), "dSigma0 block %ld is not symmetric", k);
      }
  {      /* NULL seeds are seeds of zeros; a NULL dSigma0 changes nothing else */
    double* zeros = (double*)calloc(qX + nS, sizeof(double));
    double* b2 = (double*)malloc(sizeof(double) * nAll);
    BLOCKS(b2, qmb, qcb, qxb, qdb, qsb, tb, sb, dub, dxb, dsb);
    (void)dsb;
    CHECK_GPK(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, NULL, NULL, qda, qsa));
    CHECK_GPK(VJP(dKi, Np, Np, P, Xq, Sq, R, qmb, qcb, qxb, gm, zeros, zeros, qdb, qsb));
    EXPECT(!memcmp(qda, qdb, sizeof(double) * (qD + qS)), "gpk_moments_vjp_host: NULL seeds differ from zero seeds");
    CHECK_GPK(GRAD(dKi, Np, R, H, x0, R, U, R, S0, ta, sa, gx, NULL, dua, dxa, dsa));
    CHECK_GPK(GRAD(dKi, Np, R, H, x0, R, U, R, S0, tb, sb, gx, zeros, dub, dxb, NULL));
    EXPECT(!memcmp(dua, dub, sizeof(double) * (nU + nx0)), "gpk_propagate_mm_grad_host: a NULL gS differs from zeros, or a NULL dSigma0 changed dU");
    free(zeros);
    free(b2);
  }

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
#define MVJP(B_, nx_, ish_, isc_, M_, m_, c_, x_, gm_, d_, s_) \
  gpk_moments_vjp_host_multi(h, B_, Xs, As, N, D, lsB, sf2B, ym, ys, Ks, Np, Np, kssB, 0.0, 1, noiseB, nx_, ish_, isc_, Xq, Sq, M_, m_, c_, x_, gm_, gc, gxc, d_, s_)
#define MGRAD(B_, nx_, coord_, ish_, isc_, R_, H_, t_, s_, gx_, du_, dx_, ds_) \
  gpk_propagate_mm_grad_host_multi(h, B_, Xs, As, N, D, lsB, sf2B, ym, ys, Ks, Np, Np, kssB, 0.0, 1, noiseB, nx_, coord_, ish_, isc_, x0, R, U, R, lin, S0, 1, Q, R_, H_, t_, s_, NULL, NULL, NULL, gx_, gS, du_, dx_, ds_)
  CHECK_GPK(MVJP(B, P, ish, isc, R, qm2, qc2, qx2, gm, qd2, qs2));
  CHECK_GPK(MGRAD(B, P, coord, ish, isc, R, H, t2, s2, gx, du2, dx2, ds2));
  for (size_t i = nAll; i < 2 * nAll; ++i) EXPECT(isfinite(out[i]), "multi: out[%zu] is not finite", i);
  for (size_t i = 0; i < nAll; ++i) again[i] = NAN;
  CHECK_GPK(MVJP(B, P, ish, isc, R, qma, qca, qxa, gm, qda, qsa));
  CHECK_GPK(MGRAD(B, P, coord, ish, isc, R, H, ta, sa, gx, dua, dxa, dsa));
  EXPECT(!memcmp(again, out + nAll, sizeof(double) * nAll), "multi: two calls differ");
  CHECK_GPK(gpk_moments_host_multi(h, B, Xs, As, N, D, lsB, sf2B, ym, ys, Ks, Np, Np, kssB, 0.0, 1, noiseB, P, ish, isc, Xq, Sq, R, qmf, qcf, qxf));
  CHECK_GPK(gpk_propagate_mm_host_multi(h, B, Xs, As, N, D, lsB, sf2B, ym, ys, Ks, Np, Np, kssB, 0.0, 1, noiseB, P, coord, ish, isc, x0, R, U,
                                        R, lin, S0, 1, Q, R, H, tf, sf, NULL, NULL, NULL));
  EXPECT(!memcmp(qm2, qmf, sizeof(double) * (qM + qC + qX)), "gpk_moments_vjp_host_multi: not the bits of gpk_moments_host_multi");
  EXPECT(!memcmp(t2, tf, sizeof(double) * (nT + nS)), "gpk_propagate_mm_grad_host_multi: not the bits of gpk_propagate_mm_host_multi");

  /* ---- bad arguments: statuses before any launch, the outputs untouched ---------------------------------------------------------- */
  for (size_t i = 0; i < nAll; ++i) memcpy(again + i, &canary, sizeof(double));
  BAD(gpk_moments_vjp_host(NULL, dX, dA, N, D, P, ls, sf2, ym, ys, dKi, Np, Np, kss, 0.0, 0, 0.0, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa), "null handle");
  BAD(VJP(NULL, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: null K^-1");
  EXPECT(strstr(gpk_last_error(h), "K^-1") != NULL, "message: %s", gpk_last_error(h));
  BAD(VJP(dKi, Np, Np - 1, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: ldk < Np");
  BAD(VJP(dKi, Np + 128, Np + 128, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: Np != gpk_padded(N)");
  BAD(VJP(dKi, Np, Np, P, Xq, Sq, 0, qma, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: M = 0");
  BAD(VJP(dKi, Np, Np, P, Xq, Sq, 33, qma, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: M = 33");
  EXPECT(strstr(gpk_last_error(h), "M must be in [1, 32]") != NULL, "message: %s", gpk_last_error(h));
  BAD(VJP(dKi, Np, Np, D + 1, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: nx > D");
  BAD(VJP(dKi, Np, Np, P, NULL, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: null queries");
  BAD(VJP(dKi, Np, Np, P, Xq, Sq, R, NULL, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: null mean");
  BAD(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, NULL, qsa), "vjp: null dXq");
  EXPECT(strstr(gpk_last_error(h), "null result dXq or dSq") != NULL, "message: %s", gpk_last_error(h));
  BAD(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, NULL), "vjp: null dSq");
  BAD(GRAD(NULL, Np, R, H, x0, R, U, R, S0, ta, sa, gx, gS, dua, dxa, dsa), "grad: null K^-1");
  BAD(GRAD(dKi, Np - 1, R, H, x0, R, U, R, S0, ta, sa, gx, gS, dua, dxa, dsa), "grad: ldk < Np");
  BAD(GRAD(dKi, Np, 33, H, x0, 1, U, 1, S0, ta, sa, gx, gS, dua, dxa, dsa), "grad: R = 33");
  EXPECT(strstr(gpk_last_error(h), "R must be in [1, 32]") != NULL, "message: %s", gpk_last_error(h));
  BAD(GRAD(dKi, Np, R, 0, x0, R, U, R, S0, ta, sa, gx, gS, dua, dxa, dsa), "grad: H = 0");
  BAD(GRAD(dKi, Np, R, 257, x0, R, U, R, S0, ta, sa, gx, gS, dua, dxa, dsa), "grad: H = 257");
  BAD(GRAD(dKi, Np, R, H, NULL, R, U, R, S0, ta, sa, gx, gS, dua, dxa, dsa), "grad: null x0");
  BAD(GRAD(dKi, Np, R, H, x0, R, NULL, R, S0, ta, sa, gx, gS, dua, dxa, dsa), "grad: null U with D > P");
  BAD(GRAD(dKi, Np, R, H, x0, R, U, R, S0, NULL, sa, gx, gS, dua, dxa, dsa), "grad: null traj");
  BAD(GRAD(dKi, Np, R, H, x0, R, U, R, S0, ta, sa, NULL, gS, dua, dxa, dsa), "grad: null gx");
  EXPECT(strstr(gpk_last_error(h), "null seed gx or null result dx0") != NULL, "message: %s", gpk_last_error(h));
  BAD(GRAD(dKi, Np, R, H, x0, R, U, R, S0, ta, sa, gx, gS, dua, NULL, dsa), "grad: null dx0");
  BAD(GRAD(dKi, Np, R, H, x0, R, U, R, S0, ta, sa, gx, gS, NULL, dxa, dsa), "grad: null dU with D > P");
  EXPECT(strstr(gpk_last_error(h), "null result dU") != NULL, "message: %s", gpk_last_error(h));
  {
    double* bad = (double*)malloc(sizeof(double) * (nS > qX ? nS : qX));
    double bs[64];
    memcpy(bad, gm, sizeof(double) * qM); bad[qM - 1] = NAN;
    BAD(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, bad, gc, gxc, qda, qsa), "vjp: NaN in gmean");
    EXPECT(strstr(gpk_last_error(h), "seeds gmean, gcov and gxcov must not contain NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    memcpy(bad, gc, sizeof(double) * qC); bad[0] = INFINITY;
    BAD(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, bad, gxc, qda, qsa), "vjp: infinity in gcov");
    memcpy(bad, gxc, sizeof(double) * qX); bad[qX - 1] = NAN;
    BAD(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, gc, bad, qda, qsa), "vjp: NaN in gxcov");
    memcpy(bad, gm, sizeof(double) * qM); bad[0] = NAN;
    BAD(MVJP(B, P, ish, isc, R, qma, qca, qxa, bad, qda, qsa), "multi vjp: NaN in gmean");
    memcpy(bad, gx, sizeof(double) * nT); bad[nT - 1] = NAN;
    BAD(GRAD(dKi, Np, R, H, x0, R, U, R, S0, ta, sa, bad, gS, dua, dxa, dsa), "grad: NaN in gx");
    EXPECT(strstr(gpk_last_error(h), "seeds gx and gS must not contain NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    BAD(MGRAD(B, P, coord, ish, isc, R, H, ta, sa, bad, dua, dxa, dsa), "multi grad: NaN in gx");
    memcpy(bad, gS, sizeof(double) * nS); bad[0] = INFINITY;
    BAD(GRAD(dKi, Np, R, H, x0, R, U, R, S0, ta, sa, gx, bad, dua, dxa, dsa), "grad: infinity in gS");
    memcpy(bs, S0, sizeof(double) * P * P); bs[P * P - 1] = INFINITY;
    BAD(GRAD(dKi, Np, R, H, x0, R, U, R, bs, ta, sa, gx, gS, dua, dxa, dsa), "grad: infinity in Sigma0");
    EXPECT(strstr(gpk_last_error(h), "Sigma0 must not contain NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    free(bad);
  }
  {
    int twice[8] = {0, 0, 2, 3, 4, 5, 6, 7};
    double zero_scale[16];
    memcpy(zero_scale, isc, sizeof(double) * D); zero_scale[D - 1] = 0.0;
    BAD(MVJP(0, P, ish, isc, R, qma, qca, qxa, gm, qda, qsa), "multi vjp: B = 0");
    BAD(MVJP(9, P, ish, isc, R, qma, qca, qxa, gm, qda, qsa), "multi vjp: B = 9");
    BAD(MVJP(B, P, ish, NULL, R, qma, qca, qxa, gm, qda, qsa), "multi vjp: in_shift without in_scale");
    BAD(MVJP(B, P, ish, zero_scale, R, qma, qca, qxa, gm, qda, qsa), "multi vjp: in_scale = 0");
    BAD(MVJP(B, P, ish, isc, R, qma, qca, qxa, gm, NULL, qsa), "multi vjp: null dXq");
    BAD(MGRAD(B, P, twice, ish, isc, R, H, ta, sa, gx, dua, dxa, dsa), "multi grad: coord repeated");
    EXPECT(strstr(gpk_last_error(h), "distinct") != NULL, "message: %s", gpk_last_error(h));
    BAD(MGRAD(B, P, NULL, ish, isc, R, H, ta, sa, gx, dua, dxa, dsa), "multi grad: null coord");
    BAD(MGRAD(B, B - 1, coord, ish, isc, R, H, ta, sa, gx, dua, dxa, dsa), "multi grad: nx < B");
    BAD(MGRAD(B, P, coord, ish, isc, R, H, ta, sa, NULL, dua, dxa, dsa), "multi grad: null gx");
    Ks[B - 1] = NULL;
    BAD(MVJP(B, P, ish, isc, R, qma, qca, qxa, gm, qda, qsa), "multi vjp: null K^-1 of the last model");
    BAD(MGRAD(B, P, coord, ish, isc, R, H, ta, sa, gx, dua, dxa, dsa), "multi grad: null K^-1 of the last model");
    EXPECT(strstr(gpk_last_error(h), "K^-1") != NULL, "message: %s", gpk_last_error(h));
    Ks[B - 1] = dKi;
  }
  CHECK_GPK(gpk_batch_begin(h, 2));
  BAD(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa), "vjp: batched mode");
  BAD(GRAD(dKi, Np, R, H, x0, R, U, R, S0, ta, sa, gx, gS, dua, dxa, dsa), "grad: batched mode");
  CHECK_GPK(gpk_batch_end(h));
  /* after all the refusals the entries still serve */
  CHECK_GPK(VJP(dKi, Np, Np, P, Xq, Sq, R, qma, qca, qxa, gm, gc, gxc, qda, qsa));
  EXPECT(!memcmp(qda, qd1, sizeof(double) * (qD + qS)), "vjp after the refusals: the bits changed");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), 2 * nAll, f) != 2 * nAll) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  gpk_destroy(h);
  printf("moments gradient from C: OK\n");
  return 0;
}
