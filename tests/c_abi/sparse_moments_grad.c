/* gpk_sparse_moments_vjp[_multi] and gpk_sparse_propagate_mm_grad[_multi] from a plain C caller - no Python, no torch: B handles,
 * each gpk_sparse_begin -> update -> finalize, then the batch entries on all of them (latent variances, both scalers) and the
 * single entries on handle 0 (a state of one coordinate, D - 1 controls, the noise level included).
 * The pytest wrapper (tests/test_gpu_sparse_moments_grad_c_abi.py) dumps the inputs as one flat file of doubles, argv[1] - the
 * layout of tests/c_abi/sparse_moments.c with the seeds behind it:
 *   [B, n, m, D, R, H, nx]  per model: X (n x D) y (n) Z (m x D) ls (D) [sf2, noise, alpha, jitter_uu, y_mean, y_std]
 *   coord (B)  in_shift (D)  in_scale (D)  out_shift (B)  out_scale (B)
 *   x0 (R x nx)  U (R x H x (D - nx))  lin (nx x D)  Sigma0 (nx x nx)  Q (nx x nx)
 *   x0s (R x 1)  Us (R x H x (D - 1))  lins (1 x D)  Sigma0s (1)  Qs (1)
 *   gmean (R x B)  gcov (R x B x B)  gxcov (R x B x D)  gx ((H + 1) x R x nx)  gS ((H + 1) x R x nx x nx)
 *   gmeans (R)  gcovs (R)  gxcovs (R x D)  gxs ((H + 1) x R)  gSs ((H + 1) x R)
 * and compares what this program writes to argv[2] with the dense NumPy adjoint:
 *   multi:  dXq (R x D)  dSq (R x nx x nx)  traj ((H + 1) x R x nx)  Sigma ((H + 1) x R x nx x nx)  dU (R x H x (D - nx))
 *           dx0 (R x nx)  dSigma0 (R x nx x nx)
 *   single: the same seven blocks with nx = 1
 * The program itself checks that mean, cov, xcov, traj, Sigma and the stage outputs have the bits of the forward entries, that
 * repeated calls repeat their bits, that NULL seeds are zero seeds, that NULL stage outputs and a NULL dSigma0 change nothing else,
 * that the sweep without the tape (option moments_tape_mb = 0) has the same bits, and every bad-argument status with its outputs
 * untouched.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define MAXB 8
#define CHECK_GPK(hh, x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(hh)); return 3; } } while (0)
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 4; } } while (0)
#define BAD(call, what) EXPECT((call) == GPK_BAD_ARG, what)

static double* filled(size_t n, double v) {
  double* p = (double*)malloc(sizeof(double) * (n ? n : 1));
  for (size_t i = 0; i < n; ++i) p[i] = v;
  return p;
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
  const int B = (int)buf[0], D = (int)buf[3], R = (int)buf[4], H = (int)buf[5], nx = (int)buf[6];
  const long n = (long)buf[1], m = (long)buf[2];
  EXPECT(B >= 2 && B <= MAXB && D >= 2 && D <= 16 && nx >= B && nx < D && R >= 3 && R <= 32 && H >= 1 && H <= 256, "file header");
  const long per_model = n * D + n + m * D + D + 6, nu = D - nx;
  const double* coord_d = buf + 7 + B * per_model;
  const double *ish = coord_d + B, *isc = ish + D, *osh = isc + D, *osc = osh + B, *x0 = osc + B;
  const double *U = x0 + (long)R * nx, *lin = U + (long)R * H * nu, *S0 = lin + (long)nx * D, *Q = S0 + nx * nx, *x0s = Q + nx * nx;
  const double *Us = x0s + R, *lins = Us + (long)R * H * (D - 1), *S0s = lins + D, *Qs = S0s + 1;
  const size_t qM = (size_t)R * B, qC = qM * B, qX = qM * D, nGx = (size_t)(H + 1) * R * nx, nGS = nGx * nx, sG = (size_t)(H + 1) * R;
  const double *gm = Qs + 1, *gc = gm + qM, *gxc = gc + qC, *gx = gxc + qX, *gS = gx + nGx;
  const double *gms = gS + nGS, *gcs = gms + R, *gxcs = gcs + R, *gxs = gxcs + (size_t)R * D, *gSs = gxs + sG;
  EXPECT((gSs + sG - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  int coord[MAXB];
  for (int b = 0; b < B; ++b) coord[b] = (int)coord_d[b];

  gpk_handle hs[MAXB] = {NULL};
  for (int b = 0; b < B; ++b) {
    if (gpk_create(&hs[b], 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
    CHECK_GPK(hs[b], gpk_set_stream(hs[b], GPK_OWN_STREAM));
    CHECK_GPK(hs[b], gpk_set_option(hs[b], "debug_fill", 1));
  }
  gpk_handle h = hs[0];      /* the serving handle: one of the models */

  /* the Gaussian queries of the query entries: row r = [x0[r], U[r][0]] with covariance Sigma0 */
  double *Xq = filled((size_t)R * D, 0.0), *Sq = filled((size_t)R * nx * nx, 0.0), *Xqs = filled((size_t)R * D, 0.0), *Sqs = filled(R, 0.0);
  for (int r = 0; r < R; ++r) {
    memcpy(Xq + (long)r * D, x0 + (long)r * nx, sizeof(double) * nx);
    memcpy(Xq + (long)r * D + nx, U + (long)r * H * nu, sizeof(double) * nu);
    memcpy(Sq + (long)r * nx * nx, S0, sizeof(double) * nx * nx);
    Xqs[(long)r * D] = x0s[r];
    memcpy(Xqs + (long)r * D + 1, Us + (long)r * H * (D - 1), sizeof(double) * (D - 1));
    Sqs[r] = S0s[0];
  }

  /* one result set: dXq, dSq, traj, Sigma, dU, dx0, dSigma0 */
  const size_t nDX = (size_t)R * D, nDS = (size_t)R * nx * nx, nT = (size_t)(H + 1) * R * nx, nS = nT * nx, nDU = (size_t)R * H * nu;
  const size_t nD0 = (size_t)R * nx, nMulti = nDX + nDS + nT + nS + nDU + nD0 + nDS;
  const size_t sDU = (size_t)R * H * (D - 1), nSingle = nDX + R + 2 * sG + sDU + 2 * (size_t)R;
  double* out = filled(nMulti + nSingle, NAN);
  double* again = filled(nMulti, NAN);
  double *dx1 = out, *ds1 = dx1 + nDX, *t1 = ds1 + nDS, *s1 = t1 + nT, *du1 = s1 + nS, *d01 = du1 + nDU, *dS01 = d01 + nD0;
  double *dx2 = out + nMulti, *ds2 = dx2 + nDX, *t2 = ds2 + R, *s2 = t2 + sG, *du2 = s2 + sG, *d02 = du2 + sDU, *dS02 = d02 + R;
  double *dxa = again, *dsa = dxa + nDX, *ta = dsa + nDS, *sa = ta + nT, *dua = sa + nS, *d0a = dua + nDU, *dS0a = d0a + nD0;
  /* the forward entries' results, and the gradient entries' copies of them */
  const size_t nM = (size_t)H * R * B, nC = nM * B, nXc = nM * D;
  double *fm = filled(qM, NAN), *fc = filled(qC, NAN), *fx = filled(qX, NAN), *vm = filled(qM, NAN), *vc = filled(qC, NAN), *vx = filled(qX, NAN);
  double *ft = filled(nT, NAN), *fs = filled(nS, NAN), *fsm = filled(nM, NAN), *fsc = filled(nC, NAN), *fsx = filled(nXc, NAN);
  double *gsm = filled(nM, NAN), *gsc = filled(nC, NAN), *gsx = filled(nXc, NAN);

#define MVJP(nx_, Xq_, M_, m_, c_, x_, gm_, gc_, gxc_, dx_, ds_) \
  gpk_sparse_moments_vjp_multi(h, B, hs, 0, nx_, ish, isc, osh, osc, Xq_, Sq, M_, m_, c_, x_, gm_, gc_, gxc_, dx_, ds_)
#define MGRAD(nx_, coord_, R_, H_, xr_, t_, s_, m_, c_, x_, gx_, gS_, du_, d0_, dS0_) \
  gpk_sparse_propagate_mm_grad_multi(h, B, hs, 0, nx_, coord_, ish, isc, osh, osc, x0, xr_, U, xr_, lin, S0, 1, Q, R_, H_, t_, s_, m_, c_, x_, \
                                     gx_, gS_, du_, d0_, dS0_)
#define VJP(nx_, Xq_, M_, m_, c_, x_, gm_, gc_, gxc_, dx_, ds_) \
  gpk_sparse_moments_vjp(h, 1, nx_, Xq_, Sqs, M_, m_, c_, x_, gm_, gc_, gxc_, dx_, ds_)
#define GRAD(R_, H_, xr_, t_, s_, gx_, gS_, du_, d0_, dS0_) \
  gpk_sparse_propagate_mm_grad(h, 1, x0s, xr_, Us, xr_, lins, S0s, 1, Qs, R_, H_, t_, s_, NULL, NULL, NULL, gx_, gS_, du_, d0_, dS0_)

  /* ---- refusals before the models exist ------------------------------------------------------------------------------------ */
  BAD(VJP(1, Xqs, R, vm, vc, vx, gms, gcs, gxcs, dx2, ds2), "single vjp without a model");
  BAD(GRAD(R, H, R, t2, s2, gxs, gSs, du2, d02, dS02), "single chain without a model");
  BAD(MVJP(nx, Xq, R, vm, vc, vx, gm, gc, gxc, dxa, dsa), "multi vjp without models");
  BAD(MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a), "multi chain without models");
  for (int b = 0; b < B; ++b) {
    const double* X = buf + 7 + b * per_model;
    const double *y = X + n * D, *Z = y + n, *ls = Z + m * D, *hy = ls + D;
    int info = 0;
    CHECK_GPK(hs[b], gpk_sparse_begin(hs[b], Z, m, D, 1, ls, D, hy[0], hy[1], hy[2], hy[3], hy + 4, hy + 5));
    CHECK_GPK(hs[b], gpk_sparse_update(hs[b], X, y, n));
    CHECK_GPK(hs[b], gpk_sparse_finalize(hs[b], &info));
  }
  for (size_t i = 0; i < nMulti + nSingle; ++i) EXPECT(isnan(out[i]), "a refused call wrote out[%zu]", i);
  for (size_t i = 0; i < nMulti; ++i) EXPECT(isnan(again[i]), "a refused call wrote again[%zu]", i);

  /* ---- the batch entries ------------------------------------------------------------------------------------------------------- */
  CHECK_GPK(h, gpk_sparse_moments_multi(h, B, hs, 0, nx, ish, isc, osh, osc, Xq, Sq, R, fm, fc, fx));
  CHECK_GPK(h, gpk_sparse_propagate_mm_multi(h, B, hs, 0, nx, coord, ish, isc, osh, osc, x0, R, U, R, lin, S0, 1, Q, R, H, ft, fs, fsm, fsc, fsx));
  CHECK_GPK(h, MVJP(nx, Xq, R, vm, vc, vx, gm, gc, gxc, dx1, ds1));
  CHECK_GPK(h, MGRAD(nx, coord, R, H, R, t1, s1, gsm, gsc, gsx, gx, gS, du1, d01, dS01));
  for (size_t i = 0; i < nMulti; ++i) EXPECT(isfinite(out[i]), "multi: out[%zu] is not finite", i);
  EXPECT(!memcmp(vm, fm, sizeof(double) * qM) && !memcmp(vc, fc, sizeof(double) * qC) && !memcmp(vx, fx, sizeof(double) * qX),
         "gpk_sparse_moments_vjp_multi: mean, cov or xcov differ from gpk_sparse_moments_multi");
  EXPECT(!memcmp(t1, ft, sizeof(double) * nT) && !memcmp(s1, fs, sizeof(double) * nS), "the gradient chain's traj or Sigma differ from the forward chain's");
  EXPECT(!memcmp(gsm, fsm, sizeof(double) * nM) && !memcmp(gsc, fsc, sizeof(double) * nC) && !memcmp(gsx, fsx, sizeof(double) * nXc),
         "the gradient chain's stage outputs differ from the forward chain's");
  for (long k = 0; k < R; ++k)
    for (int i = 0; i < nx; ++i)
      for (int j = 0; j < i; ++j) {
        EXPECT(!memcmp(ds1 + k * nx * nx + i * nx + j, ds1 + k * nx * nx + j * nx + i, sizeof(double)), "dSq block %ld is not symmetric", k);
        EXPECT(!memcmp(dS01 + k * nx * nx + i * nx + j, dS01 + k * nx * nx + j * nx + i, sizeof(double)), "dSigma0 block %ld is not symmetric", k);
      }
  /* the same bits again, with NULL stage outputs */
  CHECK_GPK(h, MVJP(nx, Xq, R, vm, vc, vx, gm, gc, gxc, dxa, dsa));
  CHECK_GPK(h, MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a));
  EXPECT(!memcmp(again, out, sizeof(double) * nMulti), "the batch entries: two calls differ");
  /* without the tape: the same bits */
  CHECK_GPK(h, gpk_set_option(h, "moments_tape_mb", 0));
  for (size_t i = nDX + nDS; i < nMulti; ++i) again[i] = NAN;
  CHECK_GPK(h, MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a));
  CHECK_GPK(h, gpk_set_option(h, "moments_tape_mb", 1024));
  EXPECT(!memcmp(again, out, sizeof(double) * nMulti), "the sweep without the tape changed bits");
  /* a NULL dSigma0 changes nothing else */
  for (size_t i = nDX + nDS; i < nMulti; ++i) again[i] = NAN;
  CHECK_GPK(h, MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, NULL));
  EXPECT(!memcmp(ta, t1, sizeof(double) * (nT + nS + nDU + nD0)), "a NULL dSigma0 changed another result");
  for (size_t i = 0; i < nDS; ++i) EXPECT(isnan(dS0a[i]), "a NULL dSigma0 was written");
  /* NULL seeds are zero seeds */
  {
    double *zc = filled(qC, 0.0), *zx = filled(qX, 0.0), *zS = filled(nGS, 0.0), *b2 = filled(nMulti, NAN);
    CHECK_GPK(h, MVJP(nx, Xq, R, vm, vc, vx, gm, NULL, NULL, dxa, dsa));
    CHECK_GPK(h, MVJP(nx, Xq, R, vm, vc, vx, gm, zc, zx, b2, b2 + nDX));
    EXPECT(!memcmp(again, b2, sizeof(double) * (nDX + nDS)), "NULL gcov and gxcov are not zero seeds");
    CHECK_GPK(h, MVJP(nx, Xq, R, vm, vc, vx, NULL, NULL, NULL, dxa, dsa));
    for (size_t i = 0; i < nDX + nDS; ++i) EXPECT(again[i] == 0.0, "no seed at all: again[%zu] is not zero", i);
    CHECK_GPK(h, MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, NULL, dua, d0a, dS0a));
    CHECK_GPK(h, MGRAD(nx, coord, R, H, R, b2 + nDX + nDS, b2 + nDX + nDS + nT, NULL, NULL, NULL, gx, zS, b2 + nDX + nDS + nT + nS,
                       b2 + nDX + nDS + nT + nS + nDU, b2 + nDX + nDS + nT + nS + nDU + nD0));
    EXPECT(!memcmp(ta, b2 + nDX + nDS, sizeof(double) * (nMulti - nDX - nDS)), "a NULL gS is not a zero seed");
    free(zc); free(zx); free(zS); free(b2);
  }

  /* ---- the single entries on handle 0 ------------------------------------------------------------------------------------------ */
  {
    double *m0 = filled(R, NAN), *c0 = filled(R, NAN), *x0f = filled((size_t)R * D, NAN), *m1 = filled(R, NAN), *c1 = filled(R, NAN);
    double *x1f = filled((size_t)R * D, NAN), *tf = filled(sG, NAN), *sf = filled(sG, NAN), *b2 = filled(nSingle, NAN);
    CHECK_GPK(h, gpk_sparse_moments(h, 1, 1, Xqs, Sqs, R, m0, c0, x0f));
    CHECK_GPK(h, gpk_sparse_propagate_mm(h, 1, x0s, R, Us, R, lins, S0s, 1, Qs, R, H, tf, sf, NULL, NULL, NULL));
    CHECK_GPK(h, VJP(1, Xqs, R, m1, c1, x1f, gms, gcs, gxcs, dx2, ds2));
    CHECK_GPK(h, GRAD(R, H, R, t2, s2, gxs, gSs, du2, d02, dS02));
    for (size_t i = 0; i < nSingle; ++i) EXPECT(isfinite(out[nMulti + i]), "single: out[%zu] is not finite", i);
    EXPECT(!memcmp(m1, m0, sizeof(double) * R) && !memcmp(c1, c0, sizeof(double) * R) && !memcmp(x1f, x0f, sizeof(double) * R * D),
           "gpk_sparse_moments_vjp: mean, cov or xcov differ from gpk_sparse_moments");
    EXPECT(!memcmp(t2, tf, sizeof(double) * sG) && !memcmp(s2, sf, sizeof(double) * sG), "gpk_sparse_propagate_mm_grad: traj or Sigma differ");
    CHECK_GPK(h, gpk_set_option(h, "moments_tape_mb", 0));
    CHECK_GPK(h, VJP(1, Xqs, R, m1, c1, x1f, gms, gcs, gxcs, b2, b2 + nDX));
    CHECK_GPK(h, GRAD(R, H, R, b2 + nDX + R, b2 + nDX + R + sG, gxs, gSs, b2 + nDX + R + 2 * sG, b2 + nDX + R + 2 * sG + sDU,
                      b2 + nDX + R + 2 * sG + sDU + R));
    CHECK_GPK(h, gpk_set_option(h, "moments_tape_mb", 1024));
    EXPECT(!memcmp(b2, out + nMulti, sizeof(double) * nSingle), "the single entries: a second call without the tape differs");
    free(m0); free(c0); free(x0f); free(m1); free(c1); free(x1f); free(tf); free(sf); free(b2);
  }

  /* ---- bad arguments: statuses, never a fault, the outputs untouched ----------------------------------------------------------- */
  for (size_t i = 0; i < nMulti; ++i) again[i] = 7.0;
  for (size_t i = 0; i < qM; ++i) vm[i] = 7.0;
  BAD(gpk_sparse_moments_vjp(NULL, 1, 1, Xqs, Sqs, R, vm, vc, vx, gms, gcs, gxcs, dxa, dsa), "null handle");
  BAD(gpk_sparse_propagate_mm_grad(NULL, 1, x0s, R, Us, R, lins, S0s, 1, Qs, R, H, ta, sa, NULL, NULL, NULL, gxs, gSs, dua, d0a, dS0a), "null handle");
  BAD(gpk_sparse_moments_vjp_multi(NULL, B, hs, 0, nx, ish, isc, osh, osc, Xq, Sq, R, vm, vc, vx, gm, gc, gxc, dxa, dsa), "null handle");
  BAD(gpk_sparse_propagate_mm_grad_multi(NULL, B, hs, 0, nx, coord, ish, isc, osh, osc, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL,
                                         gx, gS, dua, d0a, dS0a), "null handle");
  BAD(MVJP(nx, Xq, R, vm, vc, vx, gm, gc, gxc, NULL, dsa), "null dXq");
  EXPECT(strstr(gpk_last_error(h), "dXq or dSq") != NULL, "message: %s", gpk_last_error(h));
  BAD(MVJP(nx, Xq, R, vm, vc, vx, gm, gc, gxc, dxa, NULL), "null dSq");
  BAD(MVJP(nx, Xq, 33, vm, vc, vx, gm, gc, gxc, dxa, dsa), "M = 33");
  BAD(MVJP(nx, NULL, R, vm, vc, vx, gm, gc, gxc, dxa, dsa), "null Xq");
  BAD(MVJP(nx, Xq, R, NULL, vc, vx, gm, gc, gxc, dxa, dsa), "null mean");
  BAD(MVJP(D + 1, Xq, R, vm, vc, vx, gm, gc, gxc, dxa, dsa), "nx > D");
  BAD(VJP(1, Xqs, R, vm, vc, vx, gms, gcs, gxcs, NULL, dsa), "single: null dXq");
  BAD(VJP(1, Xqs, 0, vm, vc, vx, gms, gcs, gxcs, dxa, dsa), "single: M = 0");
  BAD(MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, NULL, gS, dua, d0a, dS0a), "null gx");
  EXPECT(strstr(gpk_last_error(h), "null seed gx") != NULL, "message: %s", gpk_last_error(h));
  BAD(MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, NULL, dS0a), "null dx0");
  BAD(MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, NULL, d0a, dS0a), "null dU with controls");
  EXPECT(strstr(gpk_last_error(h), "null result dU") != NULL, "message: %s", gpk_last_error(h));
  BAD(MGRAD(nx, coord, 33, H, 1, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a), "R = 33");
  BAD(MGRAD(nx, coord, R, 257, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a), "H = 257");
  BAD(MGRAD(nx, NULL, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a), "null coord");
  BAD(MGRAD(B - 1, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a), "nx < B");
  BAD(MGRAD(nx, coord, R, H, 2, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a), "x0 with 2 rows");
  BAD(GRAD(R, H, R, ta, sa, NULL, gSs, dua, d0a, dS0a), "single: null gx");
  BAD(GRAD(R, H, R, ta, sa, gxs, gSs, dua, NULL, dS0a), "single: null dx0");
  BAD(GRAD(R, H, R, NULL, sa, gxs, gSs, dua, d0a, dS0a), "single: null traj");
  {
    double* bad = filled(nGS, 0.0);
    memcpy(bad, gx, sizeof(double) * nGx);
    bad[nGx - 1] = NAN;
    BAD(MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, bad, gS, dua, d0a, dS0a), "NaN in gx");
    EXPECT(strstr(gpk_last_error(h), "seeds gx and gS") != NULL, "message: %s", gpk_last_error(h));
    memcpy(bad, gS, sizeof(double) * nGS);
    bad[0] = INFINITY;
    BAD(MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, bad, dua, d0a, dS0a), "infinity in gS");
    memcpy(bad, gm, sizeof(double) * qM);
    bad[qM - 1] = NAN;
    BAD(MVJP(nx, Xq, R, vm, vc, vx, bad, gc, gxc, dxa, dsa), "NaN in gmean");
    EXPECT(strstr(gpk_last_error(h), "seeds gmean, gcov and gxcov") != NULL, "message: %s", gpk_last_error(h));
    memcpy(bad, gc, sizeof(double) * qC);
    bad[1] = INFINITY;
    BAD(MVJP(nx, Xq, R, vm, vc, vx, gm, bad, gxc, dxa, dsa), "infinity in gcov");
    memcpy(bad, gxc, sizeof(double) * qX);
    bad[qX - 1] = NAN;
    BAD(MVJP(nx, Xq, R, vm, vc, vx, gm, gc, bad, dxa, dsa), "NaN in gxcov");
    free(bad);
  }
  CHECK_GPK(h, gpk_set_option(h, "small_path", 0));
  BAD(MVJP(nx, Xq, R, vm, vc, vx, gm, gc, gxc, dxa, dsa), "option small_path = 0");
  BAD(MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a), "option small_path = 0");
  EXPECT(strstr(gpk_last_error(h), "small_path") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(h, gpk_set_option(h, "small_path", 1));
  CHECK_GPK(h, gpk_batch_begin(h, 2));
  BAD(VJP(1, Xqs, R, vm, vc, vx, gms, gcs, gxcs, dxa, dsa), "batched mode");
  BAD(GRAD(R, H, R, ta, sa, gxs, gSs, dua, d0a, dS0a), "batched mode");
  CHECK_GPK(h, gpk_batch_end(h));
  {
    /* a model that took rows and is not assembled again: refused before Q is touched */
    const double* X = buf + 7 + (B - 1) * per_model;
    int info = 0;
    CHECK_GPK(hs[B - 1], gpk_sparse_update(hs[B - 1], X, X + n * D, n));
    BAD(MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a), "a model that took rows and is not assembled again");
    CHECK_GPK(hs[B - 1], gpk_sparse_finalize(hs[B - 1], &info));
  }
  for (size_t i = 0; i < nMulti; ++i) EXPECT(again[i] == 7.0, "a refused call wrote again[%zu]", i);
  for (size_t i = 0; i < qM; ++i) EXPECT(vm[i] == 7.0, "a refused call wrote mean[%zu]", i);
  /* Q follows the model: the last model's rows count twice now, the gradient moves; a second call repeats it */
  CHECK_GPK(h, MGRAD(nx, coord, R, H, R, ta, sa, NULL, NULL, NULL, gx, gS, dua, d0a, dS0a));
  EXPECT(memcmp(dua, du1, sizeof(double) * nDU), "the gradient did not follow the model that took rows");
  {
    double* b2 = filled(nMulti, NAN);
    CHECK_GPK(h, MGRAD(nx, coord, R, H, R, b2 + nDX + nDS, b2 + nDX + nDS + nT, NULL, NULL, NULL, gx, gS, b2 + nDX + nDS + nT + nS,
                       b2 + nDX + nDS + nT + nS + nDU, b2 + nDX + nDS + nT + nS + nDU + nD0));
    EXPECT(!memcmp(ta, b2 + nDX + nDS, sizeof(double) * (nMulti - nDX - nDS)), "after the rows: two calls differ");
    free(b2);
  }

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), nMulti + nSingle, f) != nMulti + nSingle) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  for (int b = 0; b < B; ++b) gpk_destroy(hs[b]);
  free(gsm); free(gsc); free(gsx); free(ft); free(fs); free(fsm); free(fsc); free(fsx);
  free(fm); free(fc); free(fx); free(vm); free(vc); free(vx);
  free(again); free(out); free(Sqs); free(Xqs); free(Sq); free(Xq); free(buf);
  printf("sparse moments gradient from C: OK\n");
  return 0;
}
