/* Training entries of the sparse inducing-point GP from a plain C caller - no Python, no torch: gpk_sparse_begin ->
 * gpk_sparse_hold -> gpk_sparse_eval, on the problem the pytest wrapper (tests/test_gpu_sparse_train_c_abi.py) writes as one
 * flat file of doubles (argv[1]):
 *   [N, m, D, P, sf2, noise, jitter, jitter_uu] X (N x D) Y (N x P) Z (m x D) ls (D) y_mean (P) y_std (P)
 * and whose results it reads back from argv[2] to compare them with the fixture (tests/golden/sparse_train_ref.npz, case A):
 *   bound  grad (D + 2: d/dlog [ls .., noise, sf2])
 * Here: the value-only evaluation and a second evaluation reproduce the bits, the evaluated object serves, and the status of
 * every bad-argument call - above all gpk_sparse_eval after a gpk_sparse_update, which releases the held rows.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define CHECK_GPK(x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(h)); return 3; } } while (0)
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 4; } } while (0)
#define REFUSED(x) do { int r_ = (x); EXPECT(r_ == GPK_BAD_ARG && strlen(gpk_last_error(h)) > 0, "%s -> %d: must be refused with a message", #x, r_); } while (0)

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <problem file> <result file>\n", argv[0]); return 1; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  double* buf = (double*)malloc(bytes);
  if (fread(buf, 1, bytes, f) != (size_t)bytes) { fprintf(stderr, "short read\n"); return 1; }
  fclose(f);
  const long N = (long)buf[0], m = (long)buf[1];
  const int D = (int)buf[2], P = (int)buf[3];
  const double sf2 = buf[4], noise = buf[5], jitter = buf[6], jitter_uu = buf[7];
  const double* X = buf + 8;
  const double* Y = X + N * D;
  const double* Z = Y + N * P;
  const double* ls = Z + m * D;
  const double* y_mean = ls + D;
  const double* y_std = y_mean + P;
  EXPECT((y_std + P - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  EXPECT(P <= GPK_MAX_P && D <= 16 && N > 20, "P = %d, D = %d, N = %ld", P, D, N);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));

  double out[1 + 18], again[1 + 18], mean[GPK_MAX_P], mean2[GPK_MAX_P];
  for (int i = 0; i < 19; ++i) out[i] = again[i] = NAN;
  int info = -1;
  int64_t rows = -1;

  /* nothing begun yet */
  REFUSED(gpk_sparse_hold(h, X, Y, N));
  EXPECT(strstr(gpk_last_error(h), "gpk_sparse_begin") != NULL, "message: %s", gpk_last_error(h));
  REFUSED(gpk_sparse_eval(h, ls, D, sf2, noise, out, out + 1, &info));
  CHECK_GPK(gpk_sparse_begin(h, Z, m, D, P, ls, D, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  /* no held rows yet; the refusals of gpk_sparse_hold */
  REFUSED(gpk_sparse_eval(h, ls, D, sf2, noise, out, out + 1, &info));
  EXPECT(strstr(gpk_last_error(h), "gpk_sparse_hold") != NULL, "message: %s", gpk_last_error(h));
  REFUSED(gpk_sparse_hold(h, NULL, Y, N));
  REFUSED(gpk_sparse_hold(h, X, Y, -1));
  {
    double* bad = (double*)malloc((size_t)(N * P) * sizeof(double));
    memcpy(bad, Y, (size_t)(N * P) * sizeof(double));
    bad[N * P - 1] = INFINITY;
    REFUSED(gpk_sparse_hold(h, X, bad, N));
    free(bad);
  }
  CHECK_GPK(gpk_sparse_hold(h, X, Y, 20));          /* a second hold replaces rows and statistics */
  CHECK_GPK(gpk_sparse_hold(h, X, Y, N));
  /* the refusals of gpk_sparse_eval */
  REFUSED(gpk_sparse_eval(h, NULL, D, sf2, noise, out, out + 1, &info));
  REFUSED(gpk_sparse_eval(h, ls, D, sf2, noise, NULL, out + 1, &info));
  REFUSED(gpk_sparse_eval(h, ls, D, sf2, noise, out, out + 1, NULL));
  REFUSED(gpk_sparse_eval(h, ls, D == 1 ? 2 : 1, sf2, noise, out, out + 1, &info));
  REFUSED(gpk_sparse_eval(h, ls, D, 0.0, noise, out, out + 1, &info));
  REFUSED(gpk_sparse_eval(h, ls, D, sf2, -1.0, out, out + 1, &info));
  {
    double bad[16];
    memcpy(bad, ls, (size_t)D * sizeof(double));
    bad[D - 1] = 0.0;
    REFUSED(gpk_sparse_eval(h, bad, D, sf2, noise, out, out + 1, &info));
  }

  CHECK_GPK(gpk_sparse_eval(h, ls, D, sf2, noise, out, out + 1, &info));
  EXPECT(info == 0, "info = %d", info);
  /* the evaluated object is the finalised model */
  CHECK_GPK(gpk_sparse_bound(h, again, &rows));
  EXPECT(rows == N && memcmp(again, out, sizeof(double)) == 0, "bound of the evaluated model, rows = %ld", (long)rows);
  CHECK_GPK(gpk_sparse_predict(h, X, 1, mean, NULL, 0));
  /* the value alone, then everything again: the same bits */
  CHECK_GPK(gpk_sparse_eval(h, ls, D, sf2, noise, again, NULL, &info));
  EXPECT(memcmp(again, out, sizeof(double)) == 0, "the value-only evaluation must reproduce the bound");
  CHECK_GPK(gpk_sparse_eval(h, ls, D, sf2, noise, again, again + 1, &info));
  EXPECT(memcmp(again, out, (size_t)(D + 3) * sizeof(double)) == 0, "a second evaluation must reproduce the bits");
  CHECK_GPK(gpk_sparse_predict(h, X, 1, mean2, NULL, 0));
  EXPECT(memcmp(mean, mean2, (size_t)P * sizeof(double)) == 0, "the served model after the second evaluation");
  for (int i = 0; i < D + 3; ++i) EXPECT(isfinite(out[i]), "entry %d", i);

  /* an update makes the statistics those of more rows than are held: the held rows are released */
  CHECK_GPK(gpk_sparse_update(h, X, Y, 10));
  REFUSED(gpk_sparse_eval(h, ls, D, sf2, noise, again, again + 1, &info));
  EXPECT(strstr(gpk_last_error(h), "gpk_sparse_hold") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(gpk_sparse_finalize(h, &info));         /* ... and the object goes on as before */
  CHECK_GPK(gpk_sparse_bound(h, again, &rows));
  EXPECT(rows == N + 10, "rows = %ld", (long)rows);
  CHECK_GPK(gpk_sparse_hold(h, X, Y, N));
  CHECK_GPK(gpk_sparse_hold(h, NULL, NULL, 0));     /* releases them */
  REFUSED(gpk_sparse_eval(h, ls, D, sf2, noise, again, again + 1, &info));

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)(D + 3), f) != (size_t)(D + 3)) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("bound = %.17g\nC ABI sparse train: OK\n", out[0]);
  free(buf);
  gpk_destroy(h);
  return 0;
}
