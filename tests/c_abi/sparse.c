/* The sparse inducing-point GP from a plain C caller - no Python, no torch: gpk_sparse_begin -> gpk_sparse_update x 2 ->
 * gpk_sparse_finalize -> gpk_sparse_predict -> gpk_sparse_bound -> gpk_sparse_export, then gpk_sparse_import into a second
 * handle, on the problem the pytest wrapper (tests/test_gpu_sparse_c_abi.py) writes as one flat file of doubles (argv[1]):
 *   [N, m, D, P, M, M_small, n_first, sf2, noise, jitter, jitter_uu] X (N x D) Y (N x P) Z (m x D) Xq (M x D) ls (D) y_mean (P) y_std (P)
 * and whose results it reads back from argv[2] to compare them with the fixture (tests/golden/sparse_ref.npz, case A):
 *   mean (M x P) var (M x P) [the panel path]  mean (M_small x P) var (M_small x P) [the small path]  bound  G (m x m) g (m x P) yy (P)
 * Here: the importing handle reproduces the bits, and the status of every bad-argument call.
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
  const long total = 2 * nmp + 2 * nsp + 1 + m * m + m * P + P;
  double* out = (double*)malloc((size_t)total * sizeof(double));
  double* again = (double*)malloc((size_t)total * sizeof(double));
  for (long i = 0; i < total; ++i) out[i] = again[i] = NAN;
  double *mean = out, *var = mean + nmp, *smean = var + nmp, *svar = smean + nsp, *bound = svar + nsp, *G = bound + 1,
         *g = G + m * m, *yy = g + m * P;
  int info = -1;
  int64_t rows = -1;

  /* nothing begun yet */
  REFUSED(gpk_sparse_update(h, X, Y, n1));
  EXPECT(strstr(gpk_last_error(h), "gpk_sparse_begin") != NULL, "message: %s", gpk_last_error(h));
  REFUSED(gpk_sparse_finalize(h, &info));
  REFUSED(gpk_sparse_predict(h, Xq, Ms, smean, svar, 1));
  REFUSED(gpk_sparse_bound(h, bound, &rows));
  REFUSED(gpk_sparse_export(h, NULL, NULL, NULL, NULL, NULL, G, g, yy, &rows, NULL, NULL, NULL, NULL));
  /* gpk_sparse_begin's refusals */
  REFUSED(gpk_sparse_begin(h, NULL, m, D, P, ls, D, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, 0, D, P, ls, D, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, 16385, D, P, ls, D, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, m, 17, P, ls, 1, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, m, D, GPK_MAX_P + 1, ls, D, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, m, D, P, ls, 2, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, m, D, P, ls, D, 0.0, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, m, D, P, ls, D, sf2, 0.0, 0.0, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, m, D, P, ls, D, sf2, noise, jitter, -1.0, y_mean, y_std));
  REFUSED(gpk_sparse_begin(h, Z, m, D, P, ls, D, sf2, noise, jitter, jitter_uu, y_mean, NULL));
  /* the building block's refusals (before anything is launched: the pointers are never followed) */
  REFUSED(gpk_sparse_accumulate(h, X, Y, 0, Z, m, D, P, ls, sf2, out, 512));
  REFUSED(gpk_sparse_accumulate(h, X, Y, N, Z, m, D, P, ls, sf2, NULL, 512));
  REFUSED(gpk_sparse_accumulate(h, X, Y, N, Z, m, D, P, ls, sf2, out, gpk_padded(m) + 126));
  REFUSED(gpk_sparse_accumulate(h, X, Y, N, Z, 16385, D, P, ls, sf2, out, 32768));

  CHECK_GPK(gpk_sparse_begin(h, Z, m, D, P, ls, D, sf2, noise, jitter, jitter_uu, y_mean, y_std));
  REFUSED(gpk_sparse_predict(h, Xq, Ms, smean, svar, 1));       /* not finalised yet */
  REFUSED(gpk_sparse_update(h, X, Y, 0));
  REFUSED(gpk_sparse_update(h, NULL, Y, n1));
  {
    double* bad = (double*)malloc((size_t)(n1 * D) * sizeof(double));
    memcpy(bad, X, (size_t)(n1 * D) * sizeof(double));
    bad[n1 * D - 1] = NAN;
    REFUSED(gpk_sparse_update(h, bad, Y, n1));
    free(bad);
  }
  CHECK_GPK(gpk_sparse_update(h, X, Y, n1));
  CHECK_GPK(gpk_sparse_update(h, X + n1 * D, Y + n1 * P, N - n1));
  REFUSED(gpk_sparse_finalize(h, NULL));
  CHECK_GPK(gpk_sparse_finalize(h, &info));
  EXPECT(info == 0, "info = %d", info);
  CHECK_GPK(gpk_sparse_predict(h, Xq, M, mean, var, 0));
  CHECK_GPK(gpk_sparse_predict(h, Xq, Ms, smean, svar, 0));
  CHECK_GPK(gpk_sparse_bound(h, bound, &rows));
  EXPECT(rows == N, "rows = %ld", (long)rows);
  /* means only, and the refusals of gpk_sparse_predict */
  CHECK_GPK(gpk_sparse_predict(h, Xq, Ms, again, NULL, 0));
  for (long i = 0; i < nsp; ++i) EXPECT(fabs(again[i] - smean[i]) <= 1e-12 * fabs(smean[i]) + 1e-300, "means only, entry %ld", i);
  REFUSED(gpk_sparse_predict(h, Xq, 0, smean, svar, 0));
  REFUSED(gpk_sparse_predict(h, NULL, Ms, smean, svar, 0));
  REFUSED(gpk_sparse_predict(h, Xq, Ms, NULL, svar, 0));
  {
    double* bad = (double*)malloc((size_t)(Ms * D) * sizeof(double));
    memcpy(bad, Xq, (size_t)(Ms * D) * sizeof(double));
    bad[0] = INFINITY;
    REFUSED(gpk_sparse_predict(h, bad, Ms, again, NULL, 0));
    free(bad);
  }

  /* export, import into a second handle: it only finalises, and reproduces the bits */
  int64_t em = 0, erows = 0;
  int eD = 0, eP = 0, enls = 0;
  double els[16], ehyper[4], eym[GPK_MAX_P], eys[GPK_MAX_P];
  double* eZ = (double*)malloc((size_t)(m * D) * sizeof(double));
  CHECK_GPK(gpk_sparse_export(h, &em, &eD, &eP, &enls, eZ, G, g, yy, &erows, els, ehyper, eym, eys));
  EXPECT(em == m && eD == D && eP == P && enls == D && erows == N, "exported sizes");
  EXPECT(memcmp(eZ, Z, (size_t)(m * D) * sizeof(double)) == 0 && memcmp(els, ls, (size_t)D * sizeof(double)) == 0, "exported Z / ls");
  EXPECT(ehyper[0] == sf2 && ehyper[1] == noise && ehyper[2] == jitter && ehyper[3] == jitter_uu, "exported hyper-parameters");
  for (long i = 0; i < m; ++i)
    for (long j = 0; j < i; ++j) EXPECT(memcmp(&G[i * m + j], &G[j * m + i], sizeof(double)) == 0, "G must be symmetric bit for bit");

  gpk_handle h1 = h, h2 = NULL;
  if (gpk_create(&h2, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  h = h2;
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));
  REFUSED(gpk_sparse_import(h, eZ, em, eD, eP, els, enls, ehyper[0], ehyper[1], ehyper[2], ehyper[3], eym, eys, NULL, g, yy, erows));
  REFUSED(gpk_sparse_import(h, eZ, em, eD, eP, els, enls, ehyper[0], ehyper[1], ehyper[2], ehyper[3], eym, eys, G, g, yy, -1));
  CHECK_GPK(gpk_sparse_import(h, eZ, em, eD, eP, els, enls, ehyper[0], ehyper[1], ehyper[2], ehyper[3], eym, eys, G, g, yy, erows));
  CHECK_GPK(gpk_sparse_finalize(h, &info));
  CHECK_GPK(gpk_sparse_predict(h, Xq, M, again, again + nmp, 0));
  CHECK_GPK(gpk_sparse_predict(h, Xq, Ms, again + 2 * nmp, again + 2 * nmp + nsp, 0));
  CHECK_GPK(gpk_sparse_bound(h, again + 2 * nmp + 2 * nsp, &rows));
  EXPECT(memcmp(out, again, (size_t)(2 * nmp + 2 * nsp + 1) * sizeof(double)) == 0 && rows == N,
         "the importing handle must reproduce the bits");
  CHECK_GPK(gpk_model_release(h));
  REFUSED(gpk_sparse_predict(h, Xq, Ms, again, NULL, 0));       /* released */
  gpk_destroy(h2);
  h = h1;

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)total, f) != (size_t)total) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("bound = %.17g\nC ABI sparse: OK\n", *bound);
  free(eZ); free(again); free(out); free(buf);
  gpk_destroy(h);
  return 0;
}
