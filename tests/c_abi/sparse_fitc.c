/* The FITC sparse GP from a plain C caller - no Python, no torch: gpk_sparse_begin -> gpk_sparse_set_approximation ->
 * gpk_sparse_update x 2 -> gpk_sparse_finalize -> gpk_sparse_predict -> gpk_sparse_bound -> gpk_sparse_export and
 * gpk_sparse_get_approximation, then gpk_sparse_import + gpk_sparse_restore_approximation into a second handle -> finalize ->
 * predict, on the problem the pytest wrapper (tests/test_gpu_sparse_fitc_c_abi.py) writes as one flat file of doubles (argv[1]):
 *   [N, m, D, P, M, M_small, n_first, sf2, noise, jitter, jitter_uu] X (N x D) Y (N x P) Z (m x D) Xq (M x D) ls (D) y_mean (P) y_std (P)
 * and whose results it reads back from argv[2] to compare them with the fixture (tests/golden/sparse_fitc_ref.npz, case A):
 *   mean (M x P) var (M x P) [the panel path]  mean (M_small x P) var (M_small x P) [the small path]  likelihood  sum log lambda
 *   G (m x m) g (m x P) yy (P)
 * Here: the importing handle reproduces the bits, and the refusals of the new entries.
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
  const long N = (long)buf[0], m = (long)buf[1], M = (long)buf[4], Ms = (long)buf[5], n1 = (long)buf[6];
  const int D = (int)buf[2], P = (int)buf[3];
  const double sf2 = buf[7], noise = buf[8], jitter = buf[9], jitter_uu = buf[10];
  const double* X = buf + 11;
  const double* Y = X + N * D;
  const double* Z = Y + N * P;
  const double* Xq = Z + m * D;
  const double* ls = Xq + M * D;
  const double* y_mean = ls + D;
  const double* y_std = y_mean + P;
  EXPECT((y_std + P - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  EXPECT(P <= GPK_MAX_P && Ms >= 1 && Ms <= 32 && M > 32 && n1 >= 1 && n1 < N, "P = %d, M = %ld, M_small = %ld", P, M, Ms);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));

  const long nmp = M * P, nsp = Ms * P;
  const long total = 2 * nmp + 2 * nsp + 2 + m * m + m * P + P;
  double* out = (double*)malloc((size_t)total * sizeof(double));
  double* again = (double*)malloc((size_t)total * sizeof(double));
  for (long i = 0; i < total; ++i) out[i] = again[i] = NAN;
  double *mean = out, *var = mean + nmp, *smean = var + nmp, *svar = smean + nsp, *lik = svar + nsp, *loglam = lik + 1,
         *G = loglam + 1, *g = G + m * m, *yy = g + m * P;
  int info = -1, kind = -1;
  int64_t rows = -1;

  /* nothing begun yet */
  REFUSED(gpk_sparse_set_approximation(h, GPK_SPARSE_FITC, &info));
  EXPECT(strstr(gpk_last_error(h), "gpk_sparse_begin") != NULL, "message: %s", gpk_last_error(h));
  REFUSED(gpk_sparse_get_approximation(h, &kind, loglam));
  REFUSED(gpk_sparse_restore_approximation(h, GPK_SPARSE_FITC, 0.0, &info));
  /* the building block's refusals (before anything is launched: the pointers are never followed) */
  REFUSED(gpk_sparse_accumulate_fitc(h, X, Y, 0, Z, m, D, P, ls, sf2, out, 512, out, 256, noise, out, NULL));
  REFUSED(gpk_sparse_accumulate_fitc(h, X, Y, N, Z, m, D, P, ls, sf2, out, 512, NULL, 256, noise, out, NULL));
  REFUSED(gpk_sparse_accumulate_fitc(h, X, Y, N, Z, m, D, P, ls, sf2, out, 512, out, gpk_padded(m) - 2, noise, out, NULL));
  REFUSED(gpk_sparse_accumulate_fitc(h, X, Y, N, Z, m, D, P, ls, sf2, out, 512, out, 256, 0.0, out, NULL));
  REFUSED(gpk_sparse_accumulate_fitc(h, X, Y, N, Z, m, D, P, ls, sf2, out, 512, out, 256, noise, NULL, NULL));

  CHECK_GPK(gpk_sparse_begin(h, Z, m, D, P, ls, D, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  CHECK_GPK(gpk_sparse_get_approximation(h, &kind, loglam));
  EXPECT(kind == GPK_SPARSE_DTC && *loglam == 0.0, "a new object is DTC");
  REFUSED(gpk_sparse_set_approximation(h, 2, &info));
  REFUSED(gpk_sparse_set_approximation(h, GPK_SPARSE_FITC, NULL));
  CHECK_GPK(gpk_sparse_set_approximation(h, GPK_SPARSE_FITC, &info));
  EXPECT(info == 0, "info = %d", info);
  CHECK_GPK(gpk_sparse_update(h, X, Y, n1));
  /* rows were seen: the kind stays (repeating it is fine) */
  REFUSED(gpk_sparse_set_approximation(h, GPK_SPARSE_DTC, &info));
  EXPECT(strstr(gpk_last_error(h), "rows") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(gpk_sparse_set_approximation(h, GPK_SPARSE_FITC, &info));
  CHECK_GPK(gpk_sparse_update(h, X + n1 * D, Y + n1 * P, N - n1));
  CHECK_GPK(gpk_sparse_finalize(h, &info));
  EXPECT(info == 0, "info = %d", info);
  CHECK_GPK(gpk_sparse_predict(h, Xq, M, mean, var, 0));
  CHECK_GPK(gpk_sparse_predict(h, Xq, Ms, smean, svar, 0));
  CHECK_GPK(gpk_sparse_bound(h, lik, &rows));
  EXPECT(rows == N, "rows = %ld", (long)rows);

  /* export + the kind and its scalar, import + restore into a second handle: it only finalises, and reproduces the bits */
  int64_t em = 0, erows = 0;
  int eD = 0, eP = 0, enls = 0;
  double els[16], ehyper[4], eym[GPK_MAX_P], eys[GPK_MAX_P];
  double* eZ = (double*)malloc((size_t)(m * D) * sizeof(double));
  CHECK_GPK(gpk_sparse_export(h, &em, &eD, &eP, &enls, eZ, G, g, yy, &erows, els, ehyper, eym, eys));
  CHECK_GPK(gpk_sparse_get_approximation(h, &kind, loglam));
  EXPECT(em == m && eD == D && eP == P && enls == D && erows == N && kind == GPK_SPARSE_FITC && isfinite(*loglam), "exported sizes / kind");
  for (long i = 0; i < m; ++i)
    for (long j = 0; j < i; ++j) EXPECT(memcmp(&G[i * m + j], &G[j * m + i], sizeof(double)) == 0, "G must be symmetric bit for bit");

  gpk_handle h1 = h, h2 = NULL;
  if (gpk_create(&h2, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  h = h2;
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));
  CHECK_GPK(gpk_sparse_import(h, eZ, em, eD, eP, els, enls, ehyper[0], ehyper[1], ehyper[2], ehyper[3], eym, eys, G, g, yy, erows));
  /* imported rows count as seen: the setter is refused, the restorer is the entry for them */
  REFUSED(gpk_sparse_set_approximation(h, GPK_SPARSE_FITC, &info));
  REFUSED(gpk_sparse_restore_approximation(h, GPK_SPARSE_FITC, NAN, &info));
  REFUSED(gpk_sparse_restore_approximation(h, 7, *loglam, &info));
  CHECK_GPK(gpk_sparse_restore_approximation(h, kind, *loglam, &info));
  CHECK_GPK(gpk_sparse_finalize(h, &info));
  CHECK_GPK(gpk_sparse_predict(h, Xq, M, again, again + nmp, 0));
  CHECK_GPK(gpk_sparse_predict(h, Xq, Ms, again + 2 * nmp, again + 2 * nmp + nsp, 0));
  CHECK_GPK(gpk_sparse_bound(h, again + 2 * nmp + 2 * nsp, &rows));
  CHECK_GPK(gpk_sparse_get_approximation(h, &kind, again + 2 * nmp + 2 * nsp + 1));
  EXPECT(memcmp(out, again, (size_t)(2 * nmp + 2 * nsp + 2) * sizeof(double)) == 0 && rows == N && kind == GPK_SPARSE_FITC,
         "the importing handle must reproduce the bits");
  gpk_destroy(h2);
  h = h1;

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)total, f) != (size_t)total) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("likelihood = %.17g\nC ABI sparse FITC: OK\n", *lik);
  free(eZ); free(again); free(out); free(buf);
  gpk_destroy(h);
  return 0;
}
