/* The inducing-input entries of the sparse GP's training from a plain C caller - no Python, no torch: gpk_sparse_begin ->
 * gpk_sparse_hold -> gpk_sparse_eval_z, on the problem the pytest wrapper (tests/test_gpu_sparse_z_c_abi.py) writes as one flat
 * file of doubles (argv[1]):
 *   [N, m, D, P, sf2, noise, jitter, jitter_uu] X (N x D) Y (N x P) Z (m x D) ls (D) y_mean (P) y_std (P)
 * and whose results it reads back from argv[2] to compare them with the fixtures (case A):
 *   bound  grad (D + 2: d/dlog [ls .., noise, sf2])  gradZ (m x D)
 * Here: evaluations reproduce their bits, Z == NULL is gpk_sparse_eval bit for bit, a Z given is the Z exported, and the status
 * of every bad-argument call - a Z that is not finite, and an evaluation without held rows.
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
  EXPECT(P <= GPK_MAX_P && D <= 16 && N > 20 && m > 2, "P = %d, D = %d, N = %ld, m = %ld", P, D, N, m);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));

  const size_t nz = (size_t)(m * D), nout = 1 + (size_t)D + 2 + nz;
  double* out = (double*)malloc(nout * sizeof(double));
  double* again = (double*)malloc(nout * sizeof(double));
  double* plain = (double*)malloc(nout * sizeof(double));
  double* Zx = (double*)malloc(nz * sizeof(double));
  double* Zm = (double*)malloc(nz * sizeof(double));
  for (size_t i = 0; i < nout; ++i) out[i] = again[i] = plain[i] = NAN;
  double *grad = out + 1, *gradZ = out + 1 + D + 2;
  int info = -1;
  int64_t rows = -1;

  /* nothing begun yet; begun, but no held rows */
  REFUSED(gpk_sparse_eval_z(h, Z, ls, D, sf2, noise, out, grad, gradZ, &info));
  CHECK_GPK(gpk_sparse_begin(h, Z, m, D, P, ls, D, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_eval_z(h, Z, ls, D, sf2, noise, out, grad, gradZ, &info));
  EXPECT(strstr(gpk_last_error(h), "gpk_sparse_hold") != NULL, "message: %s", gpk_last_error(h));
  REFUSED(gpk_sparse_eval_z(h, NULL, ls, D, sf2, noise, out, grad, gradZ, &info));
  CHECK_GPK(gpk_sparse_hold(h, X, Y, N));
  /* the refusals of gpk_sparse_eval_z: those of gpk_sparse_eval, and a Z that is not finite */
  REFUSED(gpk_sparse_eval_z(h, Z, NULL, D, sf2, noise, out, grad, gradZ, &info));
  REFUSED(gpk_sparse_eval_z(h, Z, ls, D, sf2, noise, NULL, grad, gradZ, &info));
  REFUSED(gpk_sparse_eval_z(h, Z, ls, D, sf2, noise, out, grad, gradZ, NULL));
  REFUSED(gpk_sparse_eval_z(h, Z, ls, D == 1 ? 2 : 1, sf2, noise, out, grad, gradZ, &info));
  REFUSED(gpk_sparse_eval_z(h, Z, ls, D, 0.0, noise, out, grad, gradZ, &info));
  memcpy(Zm, Z, nz * sizeof(double));
  Zm[nz - 1] = NAN;
  REFUSED(gpk_sparse_eval_z(h, Zm, ls, D, sf2, noise, out, grad, gradZ, &info));
  Zm[nz - 1] = INFINITY;
  REFUSED(gpk_sparse_eval_z(h, Zm, ls, D, sf2, noise, out, grad, gradZ, &info));
  /* ... a refused Z leaves the object's inducing inputs alone */
  CHECK_GPK(gpk_sparse_export(h, NULL, NULL, NULL, NULL, Zx, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));
  EXPECT(memcmp(Zx, Z, nz * sizeof(double)) == 0, "a refused call must not move Z");

  /* gpk_sparse_eval, then gpk_sparse_eval_z with Z == NULL and no gradZ: the same bits */
  CHECK_GPK(gpk_sparse_eval(h, ls, D, sf2, noise, plain, plain + 1, &info));
  EXPECT(info == 0, "info = %d", info);
  CHECK_GPK(gpk_sparse_eval_z(h, NULL, ls, D, sf2, noise, again, again + 1, NULL, &info));
  EXPECT(memcmp(again, plain, (size_t)(D + 3) * sizeof(double)) == 0, "Z == NULL, gradZ == NULL must be gpk_sparse_eval bit for bit");
  /* everything, with the Z given: bound and gradient keep those bits */
  CHECK_GPK(gpk_sparse_eval_z(h, Z, ls, D, sf2, noise, out, grad, gradZ, &info));
  EXPECT(info == 0, "info = %d", info);
  EXPECT(memcmp(out, plain, (size_t)(D + 3) * sizeof(double)) == 0, "bound and gradient beside gradZ must be gpk_sparse_eval's bits");
  for (size_t i = 0; i < nout; ++i) EXPECT(isfinite(out[i]), "entry %zu", i);
  CHECK_GPK(gpk_sparse_bound(h, again, &rows));
  EXPECT(rows == N && memcmp(again, out, sizeof(double)) == 0, "bound of the evaluated model, rows = %ld", (long)rows);
  /* again, with Z == NULL and with gradZ alone: bit-repeatable */
  for (size_t i = 0; i < nout; ++i) again[i] = NAN;
  CHECK_GPK(gpk_sparse_eval_z(h, NULL, ls, D, sf2, noise, again, again + 1, again + 1 + D + 2, &info));
  EXPECT(memcmp(again, out, nout * sizeof(double)) == 0, "a second evaluation must reproduce the bits");
  for (size_t i = 0; i < nout; ++i) again[i] = NAN;
  CHECK_GPK(gpk_sparse_eval_z(h, Z, ls, D, sf2, noise, again, NULL, again + 1 + D + 2, &info));
  EXPECT(memcmp(again + 1 + D + 2, gradZ, nz * sizeof(double)) == 0 && again[0] == out[0], "gradZ without grad must reproduce the bits");

  /* a moved Z: exported as given, the bound changes, and moving back restores every bit */
  for (size_t i = 0; i < nz; ++i) Zm[i] = Z[i] + 0.03 * cos((double)i);
  CHECK_GPK(gpk_sparse_eval_z(h, Zm, ls, D, sf2, noise, again, again + 1, again + 1 + D + 2, &info));
  EXPECT(again[0] != out[0], "the bound at a moved Z");
  CHECK_GPK(gpk_sparse_export(h, NULL, NULL, NULL, NULL, Zx, NULL, NULL, NULL, &rows, NULL, NULL, NULL, NULL));
  EXPECT(memcmp(Zx, Zm, nz * sizeof(double)) == 0 && rows == N, "export must return the Z given");
  CHECK_GPK(gpk_sparse_eval_z(h, Z, ls, D, sf2, noise, again, again + 1, again + 1 + D + 2, &info));
  EXPECT(memcmp(again, out, nout * sizeof(double)) == 0, "moving Z back must restore the bits");
  CHECK_GPK(gpk_sparse_export(h, NULL, NULL, NULL, NULL, Zx, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));
  EXPECT(memcmp(Zx, Z, nz * sizeof(double)) == 0, "export after moving back");

  /* an update releases the held rows */
  CHECK_GPK(gpk_sparse_update(h, X, Y, 10));
  REFUSED(gpk_sparse_eval_z(h, Z, ls, D, sf2, noise, again, again + 1, again + 1 + D + 2, &info));
  EXPECT(strstr(gpk_last_error(h), "gpk_sparse_hold") != NULL, "message: %s", gpk_last_error(h));

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), nout, f) != nout) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("bound = %.17g\nC ABI sparse Z: OK\n", out[0]);
  free(buf); free(out); free(again); free(plain); free(Zx); free(Zm);
  gpk_destroy(h);
  return 0;
}
