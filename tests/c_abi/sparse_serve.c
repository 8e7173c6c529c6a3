/* gpk_sparse_predict_grad / gpk_sparse_predict_cov from a plain C caller - no Python, no torch - on case A of
 * tests/golden/sparse_ref.npz: gpk_sparse_begin -> update -> finalize -> the two entries at M = 25 (the two-factor small-batch
 * kernels) and M = 40 (the panel routes).  The pytest wrapper (tests/test_gpu_sparse_serve_c_abi.py) dumps the inputs as one
 * flat file of doubles, argv[1]:
 *   [N, m, D, P, M] X (N x D) Y (N x P) Z (m x D) Xq (M x D) ls (D) [sf2, noise, alpha, jitter_uu] y_mean (P) y_std (P)
 * and compares what this program writes to argv[2] with tests/golden/sparse_serve_ref.npz: for M' = 25, then 40,
 *   mean (M' x P) var (M' x P) dmean (M' x P x D) dvar (M' x P x D) cov (P x M' x M')
 * The program itself checks that repeated calls repeat their bits, that gpk_sparse_predict's mean and var are those of
 * gpk_sparse_predict_grad bit for bit at M = 25, and every bad-argument status.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define CHECK_GPK(x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(h)); return 3; } } while (0)
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 4; } } while (0)

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
  const long N = (long)buf[0], m = (long)buf[1], M = (long)buf[4];
  const int D = (int)buf[2], P = (int)buf[3];
  const double* X = buf + 5;
  const double* Y = X + N * D;
  const double* Z = Y + N * P;
  const double* Xq = Z + m * D;
  const double* ls = Xq + M * D;
  const double* hyper = ls + D;
  const double* y_mean = hyper + 4;
  const double* y_std = y_mean + P;
  EXPECT((y_std + P - buf) * (long)sizeof(double) == bytes && M >= 40, "file layout: %ld bytes", bytes);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  CHECK_GPK(gpk_set_option(h, "debug_fill", 1));

  const size_t nm = (size_t)M * P, nj = nm * D, nc = (size_t)P * M * M, per = 2 * nm + 2 * nj + nc;
  double* out = (double*)malloc(sizeof(double) * 2 * per);
  double* rep = (double*)malloc(sizeof(double) * per);
  double *mean = rep, *var = mean + nm, *dmean = var + nm, *dvar = dmean + nj, *cov = dvar + nj;

  /* ---- refusals before a finalised model exists ---------------------------------------------------------------------- */
  EXPECT(gpk_sparse_predict_grad(h, Xq, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "grad without a model");
  EXPECT(gpk_sparse_predict_cov(h, Xq, 5, mean, cov) == GPK_BAD_ARG, "cov without a model");
  CHECK_GPK(gpk_sparse_begin(h, Z, m, D, P, ls, D, hyper[0], hyper[1], hyper[2], hyper[3], y_mean, y_std));
  CHECK_GPK(gpk_sparse_update(h, X, Y, N / 2));
  CHECK_GPK(gpk_sparse_update(h, X + (N / 2) * D, Y + (N / 2) * P, N - N / 2));
  EXPECT(gpk_sparse_predict_grad(h, Xq, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "grad before gpk_sparse_finalize");
  EXPECT(gpk_sparse_predict_cov(h, Xq, 5, mean, cov) == GPK_BAD_ARG, "cov before gpk_sparse_finalize");
  int info = 0;
  CHECK_GPK(gpk_sparse_finalize(h, &info));

  /* ---- the two entries at 25 and 40 rows, twice each ------------------------------------------------------------------- */
  const long rows[2] = {25, 40};
  size_t at = 0;
  for (int c = 0; c < 2; ++c) {
    const long Mc = rows[c];
    const size_t cm = (size_t)Mc * P, cj = cm * D, cc = (size_t)P * Mc * Mc;
    double *o_mean = out + at, *o_var = o_mean + cm, *o_dmean = o_var + cm, *o_dvar = o_dmean + cj, *o_cov = o_dvar + cj;
    at += 2 * cm + 2 * cj + cc;
    CHECK_GPK(gpk_sparse_predict_grad(h, Xq, Mc, o_mean, o_var, o_dmean, o_dvar, 1));
    CHECK_GPK(gpk_sparse_predict_grad(h, Xq, Mc, mean, var, dmean, dvar, 1));
    EXPECT(!memcmp(o_mean, mean, sizeof(double) * cm) && !memcmp(o_var, var, sizeof(double) * cm) &&
           !memcmp(o_dmean, dmean, sizeof(double) * cj) && !memcmp(o_dvar, dvar, sizeof(double) * cj),
           "gpk_sparse_predict_grad: two calls at M = %ld differ", Mc);
    /* mean + Jacobian alone */
    CHECK_GPK(gpk_sparse_predict_grad(h, Xq, Mc, mean, NULL, dmean, NULL, 1));
    EXPECT(!memcmp(o_mean, mean, sizeof(double) * cm), "gpk_sparse_predict_grad without the variance: another mean at M = %ld", Mc);
    double worst = 0.0, top = 0.0;
    for (size_t i = 0; i < cj; ++i) {
      if (fabs(dmean[i] - o_dmean[i]) > worst) worst = fabs(dmean[i] - o_dmean[i]);
      if (fabs(o_dmean[i]) > top) top = fabs(o_dmean[i]);
    }
    EXPECT(worst <= 1e-12 * top, "gpk_sparse_predict_grad without the variance: dmean off by %.2e at M = %ld", worst / top, Mc);
    if (Mc <= 32) {
      CHECK_GPK(gpk_sparse_predict(h, Xq, Mc, mean, var, 1));
      EXPECT(!memcmp(o_mean, mean, sizeof(double) * cm) && !memcmp(o_var, var, sizeof(double) * cm),
             "gpk_sparse_predict and gpk_sparse_predict_grad disagree in mean or var at M = %ld", Mc);
    }
    CHECK_GPK(gpk_sparse_predict_cov(h, Xq, Mc, mean, o_cov));
    CHECK_GPK(gpk_sparse_predict_cov(h, Xq, Mc, mean, cov));
    EXPECT(!memcmp(o_cov, cov, sizeof(double) * cc), "gpk_sparse_predict_cov: two calls at M = %ld differ", Mc);
    if (Mc <= 32) EXPECT(!memcmp(o_mean, mean, sizeof(double) * cm), "gpk_sparse_predict_cov: another mean at M = %ld", Mc);
    for (int p = 0; p < P; ++p)
      for (long a = 0; a < Mc; ++a)
        for (long b = 0; b < a; ++b)
          EXPECT(o_cov[((size_t)p * Mc + a) * Mc + b] == o_cov[((size_t)p * Mc + b) * Mc + a], "cov not symmetric at (%d, %ld, %ld)", p, a, b);
  }

  /* ---- bad arguments: statuses, never a fault ---------------------------------------------------------------------------- */
  EXPECT(gpk_sparse_predict_grad(NULL, Xq, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "null handle");
  EXPECT(gpk_sparse_predict_cov(NULL, Xq, 5, mean, cov) == GPK_BAD_ARG, "null handle");
  EXPECT(gpk_sparse_predict_grad(h, NULL, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "null queries");
  EXPECT(gpk_sparse_predict_grad(h, Xq, 5, NULL, var, dmean, dvar, 1) == GPK_BAD_ARG, "null mean");
  EXPECT(gpk_sparse_predict_grad(h, Xq, 5, mean, var, NULL, dvar, 1) == GPK_BAD_ARG, "null dmean");
  EXPECT(gpk_sparse_predict_grad(h, Xq, 5, mean, var, dmean, NULL, 1) == GPK_BAD_ARG, "var without dvar");
  EXPECT(gpk_sparse_predict_grad(h, Xq, 5, mean, NULL, dmean, dvar, 1) == GPK_BAD_ARG, "dvar without var");
  EXPECT(gpk_sparse_predict_grad(h, Xq, 0, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "empty batch");
  EXPECT(gpk_sparse_predict_cov(h, NULL, 5, mean, cov) == GPK_BAD_ARG, "null queries");
  EXPECT(gpk_sparse_predict_cov(h, Xq, 5, NULL, cov) == GPK_BAD_ARG, "null mean");
  EXPECT(gpk_sparse_predict_cov(h, Xq, 5, mean, NULL) == GPK_BAD_ARG, "null cov");
  EXPECT(gpk_sparse_predict_cov(h, Xq, 0, mean, cov) == GPK_BAD_ARG, "empty batch");
  EXPECT(gpk_sparse_predict_cov(h, Xq, 16385, mean, cov) == GPK_BAD_ARG, "too many rows");
  double* bad = (double*)malloc(sizeof(double) * 5 * D);
  memcpy(bad, Xq, sizeof(double) * 5 * D);
  bad[2 * D + 1] = NAN;
  EXPECT(gpk_sparse_predict_grad(h, bad, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "NaN query");
  bad[2 * D + 1] = INFINITY;
  EXPECT(gpk_sparse_predict_cov(h, bad, 5, mean, cov) == GPK_BAD_ARG, "infinite query");
  EXPECT(strstr(gpk_last_error(h), "NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(gpk_batch_begin(h, 2));
  EXPECT(gpk_sparse_predict_grad(h, Xq, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "batched mode");
  EXPECT(gpk_sparse_predict_cov(h, Xq, 5, mean, cov) == GPK_BAD_ARG, "batched mode");
  CHECK_GPK(gpk_batch_end(h));
  /* the refusals left the model alone */
  CHECK_GPK(gpk_sparse_predict_grad(h, Xq, 25, mean, var, dmean, dvar, 1));
  EXPECT(!memcmp(out, mean, sizeof(double) * 25 * P), "the model changed under the refused calls");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), at, f) != at) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  gpk_destroy(h);
  free(bad); free(rep); free(out); free(buf);
  printf("sparse serving from C: OK\n");
  return 0;
}
