/* gpk_sparse_predict_multi / _multi_grad / _multi_cov from a plain C caller - no Python, no torch: B handles, each
 * gpk_sparse_begin -> update -> finalize with its own kernel, noise, normalisation and inducing inputs, then the three entries at
 * M = 25 (the two-factor small-batch kernels with the model dimension) and M = 40 (model by model through the panel routes).
 * The pytest wrapper (tests/test_gpu_sparse_batch_c_abi.py) dumps the inputs as one flat file of doubles, argv[1]:
 *   [B, n, m, D, M]  per model: X (n x D) y (n) Z (m x D) ls (D) [sf2, noise, alpha, jitter_uu, y_mean, y_std]  then Xq (M x D)
 * and compares what this program writes to argv[2] with the dense NumPy form: for M' = 25, then 40,
 *   mean (M' x B) var (M' x B) dmean (M' x B x D) dvar (M' x B x D) cov (B x M' x M')
 * The program itself checks that repeated calls repeat their bits, that block b of every result is gpk_sparse_predict[_grad|_cov]
 * on handle b bit for bit, and every bad-argument status.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define MAXB 8
#define CHECK_GPK(hh, x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(hh)); return 3; } } while (0)
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
  const int B = (int)buf[0], D = (int)buf[3];
  const long n = (long)buf[1], m = (long)buf[2], M = (long)buf[4];
  const long per_model = n * D + n + m * D + D + 6;
  const double* Xq = buf + 5 + B * per_model;
  EXPECT(B >= 2 && B <= MAXB && (Xq + M * D - buf) * (long)sizeof(double) == bytes && M >= 40, "file layout: %ld bytes", bytes);

  gpk_handle hs[MAXB + 1] = {NULL};
  for (int b = 0; b < B; ++b) {
    if (gpk_create(&hs[b], 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
    CHECK_GPK(hs[b], gpk_set_stream(hs[b], GPK_OWN_STREAM));
    CHECK_GPK(hs[b], gpk_set_option(hs[b], "debug_fill", 1));
  }
  gpk_handle h = hs[0];      /* the serving handle: one of the models */

  const size_t nm = (size_t)M * B, nj = nm * D, nc = (size_t)B * M * M, per = 2 * nm + 2 * nj + nc;
  double* out = (double*)malloc(sizeof(double) * 2 * per);
  double* rep = (double*)malloc(sizeof(double) * per);
  double* one = (double*)malloc(sizeof(double) * per);
  double *mean = rep, *var = mean + nm, *dmean = var + nm, *dvar = dmean + nj, *cov = dvar + nj;
  double *a_mean = one, *a_var = a_mean + nm, *a_dmean = a_var + nm, *a_dvar = a_dmean + nj, *a_cov = a_dvar + nj;

  /* ---- refusals before the models exist / are finalised ------------------------------------------------------------------ */
  EXPECT(gpk_sparse_predict_multi(h, B, hs, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "multi without models");
  for (int b = 0; b < B; ++b) {
    const double* X = buf + 5 + b * per_model;
    const double *y = X + n * D, *Z = y + n, *ls = Z + m * D, *hy = ls + D;
    CHECK_GPK(hs[b], gpk_sparse_begin(hs[b], Z, m, D, 1, ls, D, hy[0], hy[1], hy[2], hy[3], hy + 4, hy + 5));
    CHECK_GPK(hs[b], gpk_sparse_update(hs[b], X, y, n / 2));
    CHECK_GPK(hs[b], gpk_sparse_update(hs[b], X + (n / 2) * D, y + n / 2, n - n / 2));
    if (b + 1 < B) { int info = 0; CHECK_GPK(hs[b], gpk_sparse_finalize(hs[b], &info)); }
  }
  EXPECT(gpk_sparse_predict_multi(h, B, hs, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "multi with an un-finalised model");
  EXPECT(gpk_sparse_predict_multi_grad(h, B, hs, Xq, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "grad with an un-finalised model");
  EXPECT(gpk_sparse_predict_multi_cov(h, B, hs, Xq, 5, mean, cov) == GPK_BAD_ARG, "cov with an un-finalised model");
  EXPECT(strstr(gpk_last_error(h), "finalised") != NULL, "message: %s", gpk_last_error(h));
  { int info = 0; CHECK_GPK(hs[B - 1], gpk_sparse_finalize(hs[B - 1], &info)); }

  /* ---- the three entries at 25 and 40 rows, twice each; block b against handle b alone ---------------------------------- */
  const long rows[2] = {25, 40};
  size_t at = 0;
  for (int c = 0; c < 2; ++c) {
    const long Mc = rows[c];
    const size_t cm = (size_t)Mc * B, cj = cm * D, cc = (size_t)B * Mc * Mc;
    double *o_mean = out + at, *o_var = o_mean + cm, *o_dmean = o_var + cm, *o_dvar = o_dmean + cj, *o_cov = o_dvar + cj;
    at += 2 * cm + 2 * cj + cc;
    CHECK_GPK(h, gpk_sparse_predict_multi_grad(h, B, hs, Xq, Mc, o_mean, o_var, o_dmean, o_dvar, 1));
    CHECK_GPK(h, gpk_sparse_predict_multi_grad(h, B, hs, Xq, Mc, mean, var, dmean, dvar, 1));
    EXPECT(!memcmp(o_mean, mean, sizeof(double) * cm) && !memcmp(o_var, var, sizeof(double) * cm) &&
           !memcmp(o_dmean, dmean, sizeof(double) * cj) && !memcmp(o_dvar, dvar, sizeof(double) * cj),
           "gpk_sparse_predict_multi_grad: two calls at M = %ld differ", Mc);
    CHECK_GPK(h, gpk_sparse_predict_multi(h, B, hs, Xq, Mc, mean, var, 1));
    if (Mc <= 32)
      EXPECT(!memcmp(o_mean, mean, sizeof(double) * cm) && !memcmp(o_var, var, sizeof(double) * cm),
             "gpk_sparse_predict_multi and _multi_grad disagree in mean or var at M = %ld", Mc);
    CHECK_GPK(h, gpk_sparse_predict_multi(h, B, hs, Xq, Mc, var, NULL, 1));
    EXPECT(!memcmp(var, mean, sizeof(double) * cm), "gpk_sparse_predict_multi without the variance: another mean at M = %ld", Mc);
    CHECK_GPK(h, gpk_sparse_predict_multi_cov(h, B, hs, Xq, Mc, mean, o_cov));
    CHECK_GPK(h, gpk_sparse_predict_multi_cov(h, B, hs, Xq, Mc, mean, cov));
    EXPECT(!memcmp(o_cov, cov, sizeof(double) * cc), "gpk_sparse_predict_multi_cov: two calls at M = %ld differ", Mc);
    if (Mc <= 32) EXPECT(!memcmp(o_mean, mean, sizeof(double) * cm), "gpk_sparse_predict_multi_cov: another mean at M = %ld", Mc);
    for (int b = 0; b < B; ++b) {
      CHECK_GPK(hs[b], gpk_sparse_predict_grad(hs[b], Xq, Mc, a_mean, a_var, a_dmean, a_dvar, 1));
      CHECK_GPK(hs[b], gpk_sparse_predict_cov(hs[b], Xq, Mc, a_mean, a_cov));
      for (long i = 0; i < Mc; ++i) {
        EXPECT(o_mean[i * B + b] == a_mean[i] && o_var[i * B + b] == a_var[i], "model %d, row %ld: mean or var differs from the model alone", b, i);
        EXPECT(!memcmp(o_dmean + (i * B + b) * D, a_dmean + i * D, sizeof(double) * D) &&
               !memcmp(o_dvar + (i * B + b) * D, a_dvar + i * D, sizeof(double) * D),
               "model %d, row %ld: a gradient differs from the model alone", b, i);
      }
      EXPECT(!memcmp(o_cov + (size_t)b * Mc * Mc, a_cov, sizeof(double) * Mc * Mc), "model %d: cov differs from the model alone at M = %ld", b, Mc);
      for (long i = 0; i < Mc; ++i)
        for (long j = 0; j < i; ++j)
          EXPECT(o_cov[((size_t)b * Mc + i) * Mc + j] == o_cov[((size_t)b * Mc + j) * Mc + i], "cov not symmetric at (%d, %ld, %ld)", b, i, j);
    }
  }

  /* ---- bad arguments: statuses, never a fault ---------------------------------------------------------------------------- */
  gpk_handle with_null[MAXB] = {NULL};
  memcpy(with_null, hs, sizeof(gpk_handle) * B);
  with_null[1] = NULL;
  gpk_handle many[MAXB + 1];
  for (int b = 0; b <= MAXB; ++b) many[b] = hs[b % B];
  EXPECT(gpk_sparse_predict_multi(NULL, B, hs, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "null serving handle");
  EXPECT(gpk_sparse_predict_multi(h, 0, hs, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "B = 0");
  EXPECT(gpk_sparse_predict_multi(h, MAXB + 1, many, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "B = 9");
  EXPECT(gpk_sparse_predict_multi(h, B, NULL, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "null list");
  EXPECT(gpk_sparse_predict_multi(h, B, with_null, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "null handle in the list");
  EXPECT(gpk_sparse_predict_multi_grad(h, B, with_null, Xq, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "null handle in the list");
  EXPECT(gpk_sparse_predict_multi_cov(h, B, with_null, Xq, 5, mean, cov) == GPK_BAD_ARG, "null handle in the list");
  EXPECT(gpk_sparse_predict_multi(h, B, hs, NULL, 5, mean, var, 1) == GPK_BAD_ARG, "null queries");
  EXPECT(gpk_sparse_predict_multi(h, B, hs, Xq, 5, NULL, var, 1) == GPK_BAD_ARG, "null mean");
  EXPECT(gpk_sparse_predict_multi(h, B, hs, Xq, 0, mean, var, 1) == GPK_BAD_ARG, "empty batch");
  EXPECT(gpk_sparse_predict_multi_grad(h, B, hs, Xq, 5, mean, var, NULL, dvar, 1) == GPK_BAD_ARG, "null dmean");
  EXPECT(gpk_sparse_predict_multi_grad(h, B, hs, Xq, 5, mean, var, dmean, NULL, 1) == GPK_BAD_ARG, "var without dvar");
  EXPECT(gpk_sparse_predict_multi_grad(h, B, hs, Xq, 5, mean, NULL, dmean, dvar, 1) == GPK_BAD_ARG, "dvar without var");
  EXPECT(gpk_sparse_predict_multi_grad(h, B, hs, Xq, 0, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "empty batch");
  EXPECT(gpk_sparse_predict_multi_cov(h, B, hs, Xq, 5, mean, NULL) == GPK_BAD_ARG, "null cov");
  EXPECT(gpk_sparse_predict_multi_cov(h, B, hs, Xq, 0, mean, cov) == GPK_BAD_ARG, "empty batch");
  EXPECT(gpk_sparse_predict_multi_cov(h, B, hs, Xq, 16385, mean, cov) == GPK_BAD_ARG, "too many rows");
  double* bad = (double*)malloc(sizeof(double) * 5 * D);
  memcpy(bad, Xq, sizeof(double) * 5 * D);
  bad[2 * D + 1] = NAN;
  EXPECT(gpk_sparse_predict_multi_grad(h, B, hs, bad, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "NaN query");
  bad[2 * D + 1] = INFINITY;
  EXPECT(gpk_sparse_predict_multi_cov(h, B, hs, bad, 5, mean, cov) == GPK_BAD_ARG, "infinite query");
  EXPECT(strstr(gpk_last_error(h), "NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
  /* a model of another m, and one with two outputs, on a further handle */
  {
    const double* X0 = buf + 5;
    const double *Z0 = X0 + n * D + n, *ls0 = Z0 + m * D, *hy = ls0 + D;
    const double two_mean[2] = {0.0, 0.0}, two_std[2] = {1.0, 1.0};
    gpk_handle mixed[MAXB];
    memcpy(mixed, hs, sizeof(gpk_handle) * B);
    if (gpk_create(&hs[B], 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
    int info = 0;
    CHECK_GPK(hs[B], gpk_sparse_begin(hs[B], Z0, m - 1, D, 1, ls0, D, hy[0], hy[1], hy[2], hy[3], hy + 4, hy + 5));
    CHECK_GPK(hs[B], gpk_sparse_finalize(hs[B], &info));
    mixed[1] = hs[B];
    EXPECT(gpk_sparse_predict_multi(h, B, mixed, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "another m");
    EXPECT(strstr(gpk_last_error(h), "m and D") != NULL, "message: %s", gpk_last_error(h));
    CHECK_GPK(hs[B], gpk_sparse_begin(hs[B], Z0, m, D, 2, ls0, D, hy[0], hy[1], hy[2], hy[3], two_mean, two_std));
    CHECK_GPK(hs[B], gpk_sparse_finalize(hs[B], &info));
    EXPECT(gpk_sparse_predict_multi_cov(h, B, mixed, Xq, 5, mean, cov) == GPK_BAD_ARG, "two outputs");
    EXPECT(strstr(gpk_last_error(h), "one output") != NULL, "message: %s", gpk_last_error(h));
  }
  CHECK_GPK(h, gpk_batch_begin(h, 2));
  EXPECT(gpk_sparse_predict_multi(h, B, hs, Xq, 5, mean, var, 1) == GPK_BAD_ARG, "batched mode");
  EXPECT(gpk_sparse_predict_multi_grad(h, B, hs, Xq, 5, mean, var, dmean, dvar, 1) == GPK_BAD_ARG, "batched mode");
  EXPECT(gpk_sparse_predict_multi_cov(h, B, hs, Xq, 5, mean, cov) == GPK_BAD_ARG, "batched mode");
  CHECK_GPK(h, gpk_batch_end(h));
  /* the refusals left the models and the counters alone */
  CHECK_GPK(h, gpk_sparse_predict_multi_grad(h, B, hs, Xq, 25, mean, var, dmean, dvar, 1));
  EXPECT(!memcmp(out, mean, sizeof(double) * 25 * B) && !memcmp(out + 25 * B, var, sizeof(double) * 25 * B),
         "the models changed under the refused calls");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), at, f) != at) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  for (int b = 0; b <= B; ++b) gpk_destroy(hs[b]);
  free(bad); free(one); free(rep); free(out); free(buf);
  printf("sparse batch from C: OK\n");
  return 0;
}
