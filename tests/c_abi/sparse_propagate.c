/* gpk_sparse_propagate / gpk_sparse_propagate_multi from a plain C caller - no Python, no torch: B handles, each
 * gpk_sparse_begin -> update -> finalize with its own kernel, noise, normalisation and inducing inputs, then the batch entry on all
 * of them (latent variances, both scalers) and the single entry on handle 0 (a state of one coordinate, D - 1 controls, the noise
 * level included).
 * The pytest wrapper (tests/test_gpu_sparse_propagate_c_abi.py) dumps the inputs as one flat file of doubles, argv[1]:
 *   [B, n, m, D, R, H, nx]  per model: X (n x D) y (n) Z (m x D) ls (D) [sf2, noise, alpha, jitter_uu, y_mean, y_std]
 *   coord (B)  in_shift (D)  in_scale (D)  out_shift (B)  out_scale (B)
 *   x0 (R x nx)  U (R x H x (D - nx))  lin (nx x D)  Sigma0 (nx x nx)  Q (nx x nx)
 *   x0s (R x 1)  Us (R x H x (D - 1))  lins (1 x D)  Sigma0s (1)  Qs (1)
 * and compares what this program writes to argv[2] with the dense NumPy form:
 *   multi:  traj ((H + 1) x R x nx)  Sigma ((H + 1) x R x nx x nx)  mean (H x R x B)  var (H x R x B)  jac (H x R x B x D)
 *   single: the same five blocks with nx = B = 1
 * The program itself checks that repeated calls repeat their bits, that NULL stage outputs change nothing, that Sigma is symmetric
 * bit for bit, and every bad-argument status.
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
  EXPECT((Qs + 1 - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  int coord[MAXB];
  for (int b = 0; b < B; ++b) coord[b] = (int)coord_d[b];

  gpk_handle hs[MAXB + 1] = {NULL};
  for (int b = 0; b <= B; ++b) {
    if (gpk_create(&hs[b], 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
    CHECK_GPK(hs[b], gpk_set_stream(hs[b], GPK_OWN_STREAM));
    CHECK_GPK(hs[b], gpk_set_option(hs[b], "debug_fill", 1));
  }
  gpk_handle h = hs[0];      /* the serving handle: one of the models */

  const size_t nT = (size_t)(H + 1) * R * nx, nS = nT * nx, nM = (size_t)H * R * B, nJ = nM * D, nMulti = nT + nS + 2 * nM + nJ;
  const size_t sT = (size_t)(H + 1) * R, sM = (size_t)H * R, sJ = sM * D, nSingle = 2 * sT + 2 * sM + sJ;
  double* out = (double*)malloc(sizeof(double) * (nMulti + nSingle));
  double* again = (double*)malloc(sizeof(double) * nMulti);
  for (size_t i = 0; i < nMulti + nSingle; ++i) out[i] = NAN;
  double *t1 = out, *s1 = t1 + nT, *m1 = s1 + nS, *v1 = m1 + nM, *j1 = v1 + nM;
  double *t2 = out + nMulti, *s2 = t2 + sT, *m2 = s2 + sT, *v2 = m2 + sM, *j2 = v2 + sM;
  double *ta = again, *sa = ta + nT, *ma = sa + nS, *va = ma + nM, *ja = va + nM;

#define MULTI(hs_, B_, nx_, coord_, ish_, isc_, osh_, osc_, R_, H_, x0_, xr_, U_, ur_, S0_, sr_, t_, s_, m_, v_, j_) \
  gpk_sparse_propagate_multi(h, B_, hs_, 0, nx_, coord_, ish_, isc_, osh_, osc_, x0_, xr_, U_, ur_, lin, S0_, sr_, Q, R_, H_, t_, s_, m_, v_, j_)
#define SINGLE(R_, H_, x0_, xr_, U_, ur_, lin_, S0_, sr_, Q_, t_, s_, m_, v_, j_) \
  gpk_sparse_propagate(h, 1, x0_, xr_, U_, ur_, lin_, S0_, sr_, Q_, R_, H_, t_, s_, m_, v_, j_)

  /* ---- refusals before the models exist / are finalised ------------------------------------------------------------------ */
  BAD(SINGLE(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, t2, s2, NULL, NULL, NULL), "single without a model");
  BAD(MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "multi without models");
  for (int b = 0; b < B; ++b) {
    const double* X = buf + 7 + b * per_model;
    const double *y = X + n * D, *Z = y + n, *ls = Z + m * D, *hy = ls + D;
    CHECK_GPK(hs[b], gpk_sparse_begin(hs[b], Z, m, D, 1, ls, D, hy[0], hy[1], hy[2], hy[3], hy + 4, hy + 5));
    CHECK_GPK(hs[b], gpk_sparse_update(hs[b], X, y, n));
    if (b + 1 < B) { int info = 0; CHECK_GPK(hs[b], gpk_sparse_finalize(hs[b], &info)); }
  }
  BAD(MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "multi with an un-finalised model");
  EXPECT(strstr(gpk_last_error(h), "finalised") != NULL, "message: %s", gpk_last_error(h));
  { int info = 0; CHECK_GPK(hs[B - 1], gpk_sparse_finalize(hs[B - 1], &info)); }

  /* ---- gpk_sparse_propagate_multi: the call, the same bits again, NULL stage outputs ------------------------------------------ */
  CHECK_GPK(h, MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, t1, s1, m1, v1, j1));
  for (size_t i = 0; i < nMulti; ++i) { EXPECT(isfinite(out[i]), "multi: out[%zu] is not finite", i); again[i] = NAN; }
  CHECK_GPK(h, MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, ma, va, ja));
  EXPECT(!memcmp(again, out, sizeof(double) * nMulti), "gpk_sparse_propagate_multi: two calls differ");
  for (size_t i = 0; i < nT + nS; ++i) again[i] = NAN;
  CHECK_GPK(h, MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL));
  EXPECT(!memcmp(again, out, sizeof(double) * (nT + nS)), "gpk_sparse_propagate_multi: NULL stage outputs changed traj or Sigma");
  EXPECT(!memcmp(t1, x0, sizeof(double) * R * nx), "stage 0 of the trajectory is not x0");
  for (long k = 0; k < (long)(H + 1) * R; ++k)
    for (int i = 0; i < nx; ++i)
      for (int j = 0; j < i; ++j)
        EXPECT(!memcmp(s1 + k * nx * nx + i * nx + j, s1 + k * nx * nx + j * nx + i, sizeof(double)), "Sigma block %ld is not symmetric", k);
  /* one start and one control sequence for every rollout: the rollouts agree bit for bit */
  CHECK_GPK(h, MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, 1, U, 1, NULL, 1, ta, sa, NULL, NULL, NULL));
  for (int r = 1; r < R; ++r)
    for (int k = 0; k <= H; ++k)
      EXPECT(!memcmp(ta + ((long)k * R + r) * nx, ta + (long)k * R * nx, sizeof(double) * nx), "broadcast rollouts differ at stage %d", k);

  /* ---- gpk_sparse_propagate on handle 0 ------------------------------------------------------------------------------------------ */
  CHECK_GPK(h, SINGLE(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, t2, s2, m2, v2, j2));
  for (size_t i = 0; i < nSingle; ++i) { EXPECT(isfinite(out[nMulti + i]), "single: out[%zu] is not finite", i); again[i] = NAN; }
  {
    double *tb = again, *sb = tb + sT, *mb = sb + sT, *vb = mb + sM, *jb = vb + sM;
    CHECK_GPK(h, SINGLE(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, tb, sb, mb, vb, jb));
    EXPECT(!memcmp(again, out + nMulti, sizeof(double) * nSingle), "gpk_sparse_propagate: two calls differ");
    for (size_t i = 0; i < 2 * sT; ++i) again[i] = NAN;
    CHECK_GPK(h, SINGLE(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, tb, sb, NULL, NULL, NULL));
    EXPECT(!memcmp(again, out + nMulti, sizeof(double) * 2 * sT), "gpk_sparse_propagate: NULL stage outputs changed traj or Sigma");
    /* stage 0 has the bits of gpk_sparse_predict_grad at the rows [x0s, Us[0]] */
    double* q = (double*)malloc(sizeof(double) * R * D);
    double* pg = (double*)malloc(sizeof(double) * (2 * R + 2 * (size_t)R * D));
    for (int r = 0; r < R; ++r) {
      q[(long)r * D] = x0s[r];
      memcpy(q + (long)r * D + 1, Us + (long)r * H * (D - 1), sizeof(double) * (D - 1));
    }
    CHECK_GPK(h, gpk_sparse_predict_grad(h, q, R, pg, pg + R, pg + 2 * R, pg + 2 * R + (size_t)R * D, 1));
    EXPECT(!memcmp(m2, pg, sizeof(double) * R) && !memcmp(v2, pg + R, sizeof(double) * R) &&
           !memcmp(j2, pg + 2 * R, sizeof(double) * R * D), "stage 0 differs from gpk_sparse_predict_grad");
    free(pg); free(q);
  }

  /* ---- bad arguments: statuses, never a fault ------------------------------------------------------------------------------ */
  BAD(gpk_sparse_propagate(NULL, 1, x0s, R, Us, R, lins, S0s, 1, Qs, R, H, ta, sa, NULL, NULL, NULL), "null handle");
  BAD(gpk_sparse_propagate_multi(NULL, B, hs, 0, nx, coord, ish, isc, osh, osc, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "null handle");
  BAD(SINGLE(0, H, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "R = 0");
  BAD(SINGLE(33, H, x0s, 1, Us, 1, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "R = 33");
  EXPECT(strstr(gpk_last_error(h), "R must be in [1, 32]") != NULL, "message: %s", gpk_last_error(h));
  BAD(SINGLE(R, 0, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "H = 0");
  BAD(SINGLE(R, 257, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "H = 257");
  EXPECT(strstr(gpk_last_error(h), "H must be in [1, 256]") != NULL, "message: %s", gpk_last_error(h));
  BAD(SINGLE(R, H, NULL, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "null x0");
  BAD(SINGLE(R, H, x0s, R, NULL, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "null U with D > P");
  BAD(SINGLE(R, H, x0s, R, Us, R, NULL, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "null lin");
  BAD(SINGLE(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, NULL, sa, NULL, NULL, NULL), "null traj");
  BAD(SINGLE(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, ta, NULL, NULL, NULL, NULL), "null Sigma");
  BAD(SINGLE(R, H, x0s, 2, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "x0 with 2 rows");
  BAD(SINGLE(R, H, x0s, R, Us, 2, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "U with 2 rows");
  BAD(SINGLE(R, H, x0s, R, Us, R, lins, S0s, 2, Qs, ta, sa, NULL, NULL, NULL), "Sigma0 with 2 rows");
  {
    double* bad = (double*)malloc(sizeof(double) * R);
    memcpy(bad, x0s, sizeof(double) * R);
    bad[R - 1] = NAN;
    BAD(SINGLE(R, H, bad, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "NaN in x0");
    EXPECT(strstr(gpk_last_error(h), "NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    free(bad);
  }
  {
    int twice[MAXB] = {0}, far[MAXB];
    memcpy(far, coord, sizeof(int) * B);
    far[B - 1] = nx;
    double zero_scale[16], nan_shift[16], inf_out[MAXB];
    memcpy(zero_scale, isc, sizeof(double) * D); memcpy(nan_shift, ish, sizeof(double) * D); memcpy(inf_out, osc, sizeof(double) * B);
    zero_scale[D - 1] = 0.0; nan_shift[0] = NAN; inf_out[B - 1] = INFINITY;
    gpk_handle with_null[MAXB], many[MAXB + 1], mixed[MAXB];
    memcpy(with_null, hs, sizeof(gpk_handle) * B);
    memcpy(mixed, hs, sizeof(gpk_handle) * B);
    with_null[1] = NULL;
    for (int b = 0; b <= MAXB; ++b) many[b] = hs[b % B];
    BAD(MULTI(hs, 0, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "B = 0");
    BAD(MULTI(many, 9, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "B = 9");
    BAD(MULTI(NULL, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "null list");
    BAD(MULTI(with_null, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "null handle in the list");
    BAD(MULTI(hs, B, nx, twice, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "coord repeated");
    EXPECT(strstr(gpk_last_error(h), "distinct") != NULL, "message: %s", gpk_last_error(h));
    BAD(MULTI(hs, B, nx, far, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "coord = nx");
    BAD(MULTI(hs, B, nx, NULL, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "null coord");
    BAD(MULTI(hs, B, B - 1, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "nx < B");
    BAD(MULTI(hs, B, D + 1, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "nx > D");
    BAD(MULTI(hs, B, nx, coord, ish, NULL, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "in_shift without in_scale");
    BAD(MULTI(hs, B, nx, coord, ish, isc, NULL, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "out_scale without out_shift");
    BAD(MULTI(hs, B, nx, coord, ish, zero_scale, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "in_scale = 0");
    EXPECT(strstr(gpk_last_error(h), "non-zero") != NULL, "message: %s", gpk_last_error(h));
    BAD(MULTI(hs, B, nx, coord, nan_shift, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "NaN in in_shift");
    BAD(MULTI(hs, B, nx, coord, ish, isc, osh, inf_out, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "infinity in out_scale");
    BAD(MULTI(hs, B, nx, coord, ish, isc, osh, osc, 33, H, x0, 1, U, 1, S0, 1, ta, sa, NULL, NULL, NULL), "R = 33");
    BAD(MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, 257, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "H = 257");
    BAD(MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, 2, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "x0 with 2 rows");
    /* a model of another m, and one with two outputs, on the further handle */
    const double* X0 = buf + 7;
    const double *Z0 = X0 + n * D + n, *ls0 = Z0 + m * D, *hy = ls0 + D;
    const double two_mean[2] = {0.0, 0.0}, two_std[2] = {1.0, 1.0};
    int info = 0;
    CHECK_GPK(hs[B], gpk_sparse_begin(hs[B], Z0, m - 1, D, 1, ls0, D, hy[0], hy[1], hy[2], hy[3], hy + 4, hy + 5));
    CHECK_GPK(hs[B], gpk_sparse_finalize(hs[B], &info));
    mixed[1] = hs[B];
    BAD(MULTI(mixed, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "another m");
    EXPECT(strstr(gpk_last_error(h), "m and D") != NULL, "message: %s", gpk_last_error(h));
    CHECK_GPK(hs[B], gpk_sparse_begin(hs[B], Z0, m, D, 2, ls0, D, hy[0], hy[1], hy[2], hy[3], two_mean, two_std));
    CHECK_GPK(hs[B], gpk_sparse_finalize(hs[B], &info));
    BAD(MULTI(mixed, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "two outputs");
    EXPECT(strstr(gpk_last_error(h), "one output") != NULL, "message: %s", gpk_last_error(h));
  }
  CHECK_GPK(h, gpk_set_option(h, "small_path", 0));
  BAD(SINGLE(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "option small_path = 0");
  BAD(MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "option small_path = 0");
  EXPECT(strstr(gpk_last_error(h), "small_path") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(h, gpk_set_option(h, "small_path", 1));
  CHECK_GPK(h, gpk_batch_begin(h, 2));
  BAD(SINGLE(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "batched mode");
  BAD(MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "batched mode");
  CHECK_GPK(h, gpk_batch_end(h));
  /* the refusals left the models and the counters alone: the same bits once more */
  for (size_t i = 0; i < nMulti; ++i) again[i] = NAN;
  CHECK_GPK(h, MULTI(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, ma, va, ja));
  EXPECT(!memcmp(again, out, sizeof(double) * nMulti), "gpk_sparse_propagate_multi changed under the refused calls");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), nMulti + nSingle, f) != nMulti + nSingle) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  for (int b = 0; b <= B; ++b) gpk_destroy(hs[b]);
  free(again); free(out); free(buf);
  printf("sparse propagate from C: OK\n");
  return 0;
}
