/* gpk_sparse_moments[_multi] and gpk_sparse_propagate_mm[_multi] from a plain C caller - no Python, no torch: B handles, each
 * gpk_sparse_begin -> update -> finalize with its own kernel, noise, normalisation and inducing inputs, then the batch entries on
 * all of them (latent variances, both scalers) and the single entries on handle 0 (a state of one coordinate, D - 1 controls, the
 * noise level included).
 * The pytest wrapper (tests/test_gpu_sparse_moments_c_abi.py) dumps the inputs as one flat file of doubles, argv[1] - the layout of
 * tests/c_abi/sparse_propagate.c:
 *   [B, n, m, D, R, H, nx]  per model: X (n x D) y (n) Z (m x D) ls (D) [sf2, noise, alpha, jitter_uu, y_mean, y_std]
 *   coord (B)  in_shift (D)  in_scale (D)  out_shift (B)  out_scale (B)
 *   x0 (R x nx)  U (R x H x (D - nx))  lin (nx x D)  Sigma0 (nx x nx)  Q (nx x nx)
 *   x0s (R x 1)  Us (R x H x (D - 1))  lins (1 x D)  Sigma0s (1)  Qs (1)
 * and compares what this program writes to argv[2] with the dense NumPy form:
 *   multi:  the moments at the R queries [x0, U[:, 0]] with covariance Sigma0 - mean (R x B)  cov (R x B x B)  xcov (R x B x D) -
 *           then traj ((H + 1) x R x nx)  Sigma ((H + 1) x R x nx x nx)  mean (H x R x B)  cov (H x R x B x B)  xcov (H x R x B x D)
 *   single: the same eight blocks with nx = B = 1
 * The program itself checks that repeated calls repeat their bits, that NULL stage outputs change nothing, that cov and Sigma are
 * symmetric bit for bit, that stage 0 of a chain has the bits of the moments entry, that Q follows a model that takes rows and is
 * assembled again, and every bad-argument status with its outputs untouched.
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

  /* the Gaussian queries of the moments entries: row r = [x0[r], U[r][0]] with covariance Sigma0 */
  double* Xq = (double*)malloc(sizeof(double) * R * D);
  double* Sq = (double*)malloc(sizeof(double) * R * nx * nx);
  double* Xqs = (double*)malloc(sizeof(double) * R * D);
  double* Sqs = (double*)malloc(sizeof(double) * R);
  for (int r = 0; r < R; ++r) {
    memcpy(Xq + (long)r * D, x0 + (long)r * nx, sizeof(double) * nx);
    memcpy(Xq + (long)r * D + nx, U + (long)r * H * nu, sizeof(double) * nu);
    memcpy(Sq + (long)r * nx * nx, S0, sizeof(double) * nx * nx);
    Xqs[(long)r * D] = x0s[r];
    memcpy(Xqs + (long)r * D + 1, Us + (long)r * H * (D - 1), sizeof(double) * (D - 1));
    Sqs[r] = S0s[0];
  }

  /* one result set: the moments' three blocks, then the chain's five */
  const size_t qM = (size_t)R * B, qC = qM * B, qX = qM * D;
  const size_t nT = (size_t)(H + 1) * R * nx, nS = nT * nx, nM = (size_t)H * R * B, nC = nM * B, nXc = nM * D;
  const size_t nMulti = qM + qC + qX + nT + nS + nM + nC + nXc;
  const size_t sq = (size_t)R, sT = (size_t)(H + 1) * R, sM = (size_t)H * R, sX = sM * D;
  const size_t nSingle = 2 * sq + sq * D + 2 * sT + 2 * sM + sX;
  double* out = (double*)malloc(sizeof(double) * (nMulti + nSingle));
  double* again = (double*)malloc(sizeof(double) * nMulti);
  for (size_t i = 0; i < nMulti + nSingle; ++i) out[i] = NAN;
  double *qm1 = out, *qc1 = qm1 + qM, *qx1 = qc1 + qC, *t1 = qx1 + qX, *s1 = t1 + nT, *m1 = s1 + nS, *c1 = m1 + nM, *x1 = c1 + nC;
  double *qm2 = out + nMulti, *qc2 = qm2 + sq, *qx2 = qc2 + sq, *t2 = qx2 + sq * D, *s2 = t2 + sT, *m2 = s2 + sT, *c2 = m2 + sM, *x2 = c2 + sM;
  double *qma = again, *qca = qma + qM, *qxa = qca + qC, *ta = qxa + qX, *sa = ta + nT, *ma = sa + nS, *ca = ma + nM, *xa = ca + nC;

#define MMOM(hs_, B_, nx_, ish_, isc_, osh_, osc_, Xq_, Sq_, M_, m_, c_, x_) \
  gpk_sparse_moments_multi(h, B_, hs_, 0, nx_, ish_, isc_, osh_, osc_, Xq_, Sq_, M_, m_, c_, x_)
#define MCHAIN(hs_, B_, nx_, coord_, ish_, isc_, osh_, osc_, R_, H_, x0_, xr_, U_, ur_, S0_, sr_, t_, s_, m_, c_, x_) \
  gpk_sparse_propagate_mm_multi(h, B_, hs_, 0, nx_, coord_, ish_, isc_, osh_, osc_, x0_, xr_, U_, ur_, lin, S0_, sr_, Q, R_, H_, t_, s_, m_, c_, x_)
#define MOM(nx_, Xq_, Sq_, M_, m_, c_, x_) gpk_sparse_moments(h, 1, nx_, Xq_, Sq_, M_, m_, c_, x_)
#define CHAIN(R_, H_, x0_, xr_, U_, ur_, lin_, S0_, sr_, Q_, t_, s_, m_, c_, x_) \
  gpk_sparse_propagate_mm(h, 1, x0_, xr_, U_, ur_, lin_, S0_, sr_, Q_, R_, H_, t_, s_, m_, c_, x_)

  /* ---- refusals before the models exist / are finalised ------------------------------------------------------------------ */
  BAD(MOM(1, Xqs, Sqs, R, qm2, qc2, qx2), "single moments without a model");
  BAD(CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, t2, s2, NULL, NULL, NULL), "single chain without a model");
  BAD(MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "multi moments without models");
  for (int b = 0; b < B; ++b) {
    const double* X = buf + 7 + b * per_model;
    const double *y = X + n * D, *Z = y + n, *ls = Z + m * D, *hy = ls + D;
    CHECK_GPK(hs[b], gpk_sparse_begin(hs[b], Z, m, D, 1, ls, D, hy[0], hy[1], hy[2], hy[3], hy + 4, hy + 5));
    CHECK_GPK(hs[b], gpk_sparse_update(hs[b], X, y, n));
    if (b + 1 < B) { int info = 0; CHECK_GPK(hs[b], gpk_sparse_finalize(hs[b], &info)); }
  }
  BAD(MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "multi with an un-finalised model");
  EXPECT(strstr(gpk_last_error(h), "finalised") != NULL, "message: %s", gpk_last_error(h));
  { int info = 0; CHECK_GPK(hs[B - 1], gpk_sparse_finalize(hs[B - 1], &info)); }
  for (size_t i = 0; i < nSingle; ++i) EXPECT(isnan(out[nMulti + i]), "a refused call wrote out[%zu]", i);

  /* ---- the batch entries: the calls, the same bits again, NULL stage outputs, symmetry, stage 0 ------------------------------- */
  CHECK_GPK(h, MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, R, qm1, qc1, qx1));
  CHECK_GPK(h, MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, t1, s1, m1, c1, x1));
  for (size_t i = 0; i < nMulti; ++i) { EXPECT(isfinite(out[i]), "multi: out[%zu] is not finite", i); again[i] = NAN; }
  CHECK_GPK(h, MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa));
  CHECK_GPK(h, MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, ma, ca, xa));
  EXPECT(!memcmp(again, out, sizeof(double) * nMulti), "the batch entries: two calls differ");
  for (size_t i = 0; i < nT + nS; ++i) ta[i] = NAN;
  CHECK_GPK(h, MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL));
  EXPECT(!memcmp(ta, t1, sizeof(double) * (nT + nS)), "gpk_sparse_propagate_mm_multi: NULL stage outputs changed traj or Sigma");
  EXPECT(!memcmp(t1, x0, sizeof(double) * R * nx), "stage 0 of the trajectory is not x0");
  for (long k = 0; k < (long)(H + 1) * R; ++k)
    for (int i = 0; i < nx; ++i)
      for (int j = 0; j < i; ++j)
        EXPECT(!memcmp(s1 + k * nx * nx + i * nx + j, s1 + k * nx * nx + j * nx + i, sizeof(double)), "Sigma block %ld is not symmetric", k);
  for (long k = 0; k < (long)H * R; ++k)
    for (int i = 0; i < B; ++i)
      for (int j = 0; j < i; ++j)
        EXPECT(!memcmp(c1 + k * B * B + i * B + j, c1 + k * B * B + j * B + i, sizeof(double)), "cov block %ld is not symmetric", k);
  EXPECT(!memcmp(m1, qm1, sizeof(double) * qM) && !memcmp(c1, qc1, sizeof(double) * qC) && !memcmp(x1, qx1, sizeof(double) * qX),
         "stage 0 of the batch chain differs from gpk_sparse_moments_multi");

  /* ---- the single entries on handle 0 ------------------------------------------------------------------------------------------ */
  CHECK_GPK(h, MOM(1, Xqs, Sqs, R, qm2, qc2, qx2));
  CHECK_GPK(h, CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, t2, s2, m2, c2, x2));
  for (size_t i = 0; i < nSingle; ++i) { EXPECT(isfinite(out[nMulti + i]), "single: out[%zu] is not finite", i); again[i] = NAN; }
  {
    double *qmb = again, *qcb = qmb + sq, *qxb = qcb + sq, *tb = qxb + sq * D, *sb = tb + sT, *mb = sb + sT, *cb = mb + sM, *xb = cb + sM;
    CHECK_GPK(h, MOM(1, Xqs, Sqs, R, qmb, qcb, qxb));
    CHECK_GPK(h, CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, tb, sb, mb, cb, xb));
    EXPECT(!memcmp(again, out + nMulti, sizeof(double) * nSingle), "the single entries: two calls differ");
    for (size_t i = 0; i < 2 * sT; ++i) tb[i] = NAN;
    CHECK_GPK(h, CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, tb, sb, NULL, NULL, NULL));
    EXPECT(!memcmp(tb, t2, sizeof(double) * 2 * sT), "gpk_sparse_propagate_mm: NULL stage outputs changed traj or Sigma");
    EXPECT(!memcmp(m2, qm2, sizeof(double) * sq) && !memcmp(c2, qc2, sizeof(double) * sq) && !memcmp(x2, qx2, sizeof(double) * sq * D),
           "stage 0 of the chain differs from gpk_sparse_moments");
    /* one group of queries in the pair launch instead of the default split: the same bits */
    CHECK_GPK(h, gpk_set_option(h, "moments_query_groups", 1));
    for (size_t i = 0; i < nSingle; ++i) again[i] = NAN;
    CHECK_GPK(h, MOM(1, Xqs, Sqs, R, qmb, qcb, qxb));
    CHECK_GPK(h, CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, tb, sb, mb, cb, xb));
    CHECK_GPK(h, gpk_set_option(h, "moments_query_groups", 0));
    EXPECT(!memcmp(again, out + nMulti, sizeof(double) * nSingle), "the query split changed bits");
  }

  /* ---- bad arguments: statuses, never a fault, the outputs untouched ----------------------------------------------------------- */
  for (size_t i = 0; i < nMulti; ++i) again[i] = 7.0;
  BAD(gpk_sparse_moments(NULL, 1, 1, Xqs, Sqs, R, qma, qca, qxa), "null handle");
  BAD(gpk_sparse_propagate_mm(NULL, 1, x0s, R, Us, R, lins, S0s, 1, Qs, R, H, ta, sa, NULL, NULL, NULL), "null handle");
  BAD(gpk_sparse_moments_multi(NULL, B, hs, 0, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "null handle");
  BAD(gpk_sparse_propagate_mm_multi(NULL, B, hs, 0, nx, coord, ish, isc, osh, osc, x0, R, U, R, lin, S0, 1, Q, R, H, ta, sa, NULL, NULL, NULL), "null handle");
  BAD(MOM(1, Xqs, Sqs, 0, qma, qca, qxa), "M = 0");
  BAD(MOM(1, Xqs, Sqs, 33, qma, qca, qxa), "M = 33");
  EXPECT(strstr(gpk_last_error(h), "M must be in [1, 32]") != NULL, "message: %s", gpk_last_error(h));
  BAD(MOM(0, Xqs, Sqs, R, qma, qca, qxa), "nx = 0");
  BAD(MOM(D + 1, Xqs, Sqs, R, qma, qca, qxa), "nx > D");
  BAD(MOM(17, Xqs, Sqs, R, qma, qca, qxa), "nx = 17");
  BAD(MOM(1, NULL, Sqs, R, qma, qca, qxa), "null Xq");
  BAD(MOM(1, Xqs, Sqs, R, NULL, qca, qxa), "null mean");
  BAD(MOM(1, Xqs, Sqs, R, qma, NULL, qxa), "null cov");
  BAD(MOM(1, Xqs, Sqs, R, qma, qca, NULL), "null xcov");
  BAD(CHAIN(0, H, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "R = 0");
  BAD(CHAIN(33, H, x0s, 1, Us, 1, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "R = 33");
  EXPECT(strstr(gpk_last_error(h), "R must be in [1, 32]") != NULL, "message: %s", gpk_last_error(h));
  BAD(CHAIN(R, 0, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "H = 0");
  BAD(CHAIN(R, 257, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "H = 257");
  BAD(CHAIN(R, H, NULL, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "null x0");
  BAD(CHAIN(R, H, x0s, R, NULL, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "null U with D > P");
  BAD(CHAIN(R, H, x0s, R, Us, R, NULL, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "null lin");
  BAD(CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, NULL, sa, NULL, NULL, NULL), "null traj");
  BAD(CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, ta, NULL, NULL, NULL, NULL), "null Sigma");
  BAD(CHAIN(R, H, x0s, 2, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "x0 with 2 rows");
  BAD(CHAIN(R, H, x0s, R, Us, R, lins, S0s, 2, Qs, ta, sa, NULL, NULL, NULL), "Sigma0 with 2 rows");
  {
    double* bad = (double*)malloc(sizeof(double) * R * D);
    memcpy(bad, Xqs, sizeof(double) * R * D);
    bad[(long)R * D - 1] = NAN;
    BAD(MOM(1, bad, Sqs, R, qma, qca, qxa), "NaN in a query");
    EXPECT(strstr(gpk_last_error(h), "NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    memcpy(bad, Sqs, sizeof(double) * R);
    bad[R - 1] = INFINITY;
    BAD(MOM(1, Xqs, bad, R, qma, qca, qxa), "infinity in a covariance");
    memcpy(bad, x0s, sizeof(double) * R);
    bad[R - 1] = NAN;
    BAD(CHAIN(R, H, bad, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "NaN in x0");
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
    BAD(MMOM(hs, 0, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "B = 0");
    BAD(MMOM(many, 9, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "B = 9");
    BAD(MMOM(NULL, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "null list");
    BAD(MMOM(with_null, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "null handle in the list");
    BAD(MMOM(hs, B, D + 1, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "nx > D");
    BAD(MMOM(hs, B, nx, ish, NULL, osh, osc, Xq, Sq, R, qma, qca, qxa), "in_shift without in_scale");
    BAD(MMOM(hs, B, nx, ish, isc, NULL, osc, Xq, Sq, R, qma, qca, qxa), "out_scale without out_shift");
    BAD(MMOM(hs, B, nx, ish, zero_scale, osh, osc, Xq, Sq, R, qma, qca, qxa), "in_scale = 0");
    EXPECT(strstr(gpk_last_error(h), "non-zero") != NULL, "message: %s", gpk_last_error(h));
    BAD(MMOM(hs, B, nx, nan_shift, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "NaN in in_shift");
    BAD(MMOM(hs, B, nx, ish, isc, osh, inf_out, Xq, Sq, R, qma, qca, qxa), "infinity in out_scale");
    BAD(MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, 33, qma, qca, qxa), "M = 33");
    BAD(MCHAIN(hs, B, nx, twice, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "coord repeated");
    EXPECT(strstr(gpk_last_error(h), "distinct") != NULL, "message: %s", gpk_last_error(h));
    BAD(MCHAIN(hs, B, nx, far, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "coord = nx");
    BAD(MCHAIN(hs, B, nx, NULL, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "null coord");
    BAD(MCHAIN(hs, B, B - 1, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "nx < B");
    EXPECT(strstr(gpk_last_error(h), "number of outputs") != NULL, "message: %s", gpk_last_error(h));
    BAD(MCHAIN(hs, B, D + 1, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "nx > D");
    BAD(MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, 33, H, x0, 1, U, 1, S0, 1, ta, sa, NULL, NULL, NULL), "R = 33");
    BAD(MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, 257, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "H = 257");
    BAD(MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, 2, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "x0 with 2 rows");
    /* a model of another m, and one with two outputs, on the further handle */
    const double* X0 = buf + 7;
    const double *Z0 = X0 + n * D + n, *ls0 = Z0 + m * D, *hy = ls0 + D;
    const double two_mean[2] = {0.0, 0.0}, two_std[2] = {1.0, 1.0};
    int info = 0;
    CHECK_GPK(hs[B], gpk_sparse_begin(hs[B], Z0, m - 1, D, 1, ls0, D, hy[0], hy[1], hy[2], hy[3], hy + 4, hy + 5));
    CHECK_GPK(hs[B], gpk_sparse_finalize(hs[B], &info));
    mixed[1] = hs[B];
    BAD(MMOM(mixed, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "another m");
    EXPECT(strstr(gpk_last_error(h), "m and D") != NULL, "message: %s", gpk_last_error(h));
    CHECK_GPK(hs[B], gpk_sparse_begin(hs[B], Z0, m, D, 2, ls0, D, hy[0], hy[1], hy[2], hy[3], two_mean, two_std));
    CHECK_GPK(hs[B], gpk_sparse_finalize(hs[B], &info));
    BAD(MMOM(mixed, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "two outputs");
    EXPECT(strstr(gpk_last_error(h), "one output") != NULL, "message: %s", gpk_last_error(h));
    /* ... which the single chain refuses too: its state would be P = 2 coordinates, the horizon here has one */
  }
  CHECK_GPK(h, gpk_set_option(h, "small_path", 0));
  BAD(MOM(1, Xqs, Sqs, R, qma, qca, qxa), "option small_path = 0");
  BAD(CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "option small_path = 0");
  BAD(MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "option small_path = 0");
  BAD(MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "option small_path = 0");
  EXPECT(strstr(gpk_last_error(h), "small_path") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(h, gpk_set_option(h, "small_path", 1));
  CHECK_GPK(h, gpk_batch_begin(h, 2));
  BAD(MOM(1, Xqs, Sqs, R, qma, qca, qxa), "batched mode");
  BAD(CHAIN(R, H, x0s, R, Us, R, lins, S0s, 1, Qs, ta, sa, NULL, NULL, NULL), "batched mode");
  BAD(MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "batched mode");
  BAD(MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, NULL, NULL, NULL), "batched mode");
  CHECK_GPK(h, gpk_batch_end(h));
  for (size_t i = 0; i < nMulti; ++i) EXPECT(again[i] == 7.0, "a refused call wrote again[%zu]", i);
  /* the refusals left the models alone: the same bits once more */
  CHECK_GPK(h, MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa));
  CHECK_GPK(h, MCHAIN(hs, B, nx, coord, ish, isc, osh, osc, R, H, x0, R, U, R, S0, 1, ta, sa, ma, ca, xa));
  EXPECT(!memcmp(again, out, sizeof(double) * nMulti), "the batch entries changed under the refused calls");

  /* ---- Q follows the model: the last handle takes its own rows once more and is assembled again --------------------------------- */
  {
    const double* X = buf + 7 + (B - 1) * per_model;
    int info = 0;
    CHECK_GPK(hs[B - 1], gpk_sparse_update(hs[B - 1], X, X + n * D, n));
    BAD(MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa), "a model that took rows and is not assembled again");
    CHECK_GPK(hs[B - 1], gpk_sparse_finalize(hs[B - 1], &info));
    CHECK_GPK(h, MMOM(hs, B, nx, ish, isc, osh, osc, Xq, Sq, R, qma, qca, qxa));
    /* model 0 is untouched: its own mean, variance and input-output covariance keep their bits; the last model's moved */
    EXPECT(!memcmp(qma, qm1, sizeof(double)) && !memcmp(qca, qc1, sizeof(double)) && !memcmp(qxa, qx1, sizeof(double) * D), "model 0 changed");
    EXPECT(memcmp(qca + (size_t)B * B - 1, qc1 + (size_t)B * B - 1, sizeof(double)), "the variance of the model that took rows did not move");
  }

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), nMulti + nSingle, f) != nMulti + nSingle) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  for (int b = 0; b <= B; ++b) gpk_destroy(hs[b]);
  free(again); free(out); free(Sqs); free(Xqs); free(Sq); free(Xq); free(buf);
  printf("sparse moments from C: OK\n");
  return 0;
}
