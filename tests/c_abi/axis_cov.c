/* The per-axis covariance composite from a plain C caller - no Python, no torch: gpk_fit_batched -> gpk_predict_batched_cov on
 * the problem the pytest wrapper (tests/test_gpu_axis_cov_c_abi.py) writes as one flat file of doubles (argv[1]):
 *   [N, D, B, M, M_small, jitter] X (N x D) Y (N x B) ls (B x D) noise (B) Xq (M x D) Xq_small (M_small x D)
 * and whose results it reads back from argv[2]:
 *   the M rows (the large route: fused mean + one gpk_predict_cov_inv per model):   mean (M x B) cov (B x M x M)
 *   the M_small <= 32 rows (one gpk_predict_host_multi_cov: two launches):          mean (M_small x B) cov (B x M_small x M_small)
 * to compare them with the fixture (tests/golden/axis_cov_ref.npz, case csv) after applying the target scalers.  Here: every
 * block is symmetric bit for bit, a second call returns the same bits, and the refusals of both entries.
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define CHECK_GPK(x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(h)); return 3; } } while (0)
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 4; } } while (0)
#define REFUSED(x) do { int r_ = (x); EXPECT(r_ == GPK_BAD_ARG && strlen(gpk_last_error(h)) > 0, "%s -> %d: must be refused with a message", #x, r_); } while (0)

static int symmetric(const double* cov, int B, long M) {
  for (int b = 0; b < B; ++b)
    for (long i = 0; i < M; ++i)
      for (long j = 0; j < i; ++j)
        if (memcmp(&cov[(b * M + i) * M + j], &cov[(b * M + j) * M + i], sizeof(double)) != 0) return 0;
  return 1;
}

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
  const long N = (long)buf[0], M = (long)buf[3], Ms = (long)buf[4];
  const int D = (int)buf[1], B = (int)buf[2];
  const double jitter = buf[5];
  const double* X = buf + 6;
  const double* Y = X + N * D;
  const double* ls = Y + N * B;
  const double* noise = ls + B * D;
  const double* Xq = noise + B;
  const double* Xs = Xq + M * D;
  EXPECT((Xs + Ms * D - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  EXPECT(B <= GPK_MAX_BATCH && Ms >= 1 && Ms <= 32 && M > 32, "B = %d, M = %ld, M_small = %ld", B, M, Ms);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));

  const long nm = M * B, nc = B * M * M, sm = Ms * B, sc = B * Ms * Ms;
  const long total = nm + nc + sm + sc;
  double* out = (double*)malloc((size_t)total * sizeof(double));
  double* again = (double*)malloc((size_t)total * sizeof(double));
  for (long i = 0; i < total; ++i) out[i] = again[i] = NAN;
  double *mean = out, *cov = mean + nm, *smean = cov + nc, *scov = smean + sm;

  /* nothing fitted yet: refused */
  REFUSED(gpk_predict_batched_cov(h, Xs, Ms, smean, scov));
  EXPECT(strstr(gpk_last_error(h), "gpk_fit_batched") != NULL, "message: %s", gpk_last_error(h));

  /* the one-call entry's own refusals (every one of them before anything is launched: the pointers are never followed) */
  {
    double* dbuf = NULL;
    if (hipMalloc((void**)&dbuf, 4096) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    const double *ptr9[9], *ptrn[3];
    for (int b = 0; b < 9; ++b) ptr9[b] = dbuf;
    ptrn[0] = dbuf; ptrn[1] = NULL; ptrn[2] = dbuf;
    double one9[9], ls9[9 * 16], q33[33 * 16], m33[9 * 33], c33[9 * 33 * 33 > 1 ? 9 * 33 * 33 : 1];
    for (int i = 0; i < 9; ++i) one9[i] = 1.0;
    for (int i = 0; i < 9 * 16; ++i) ls9[i] = 1.0;
    for (int i = 0; i < 33 * 16; ++i) q33[i] = 0.0;
    const long n = 100, np_ = gpk_padded(100);
    CHECK_GPK(np_ == 128 ? GPK_OK : GPK_BAD_ARG);
    REFUSED(gpk_predict_host_multi_cov(h, 3, ptr9, ptr9, n, D, ls9, one9, one9, one9, ptr9, np_, np_, one9, q33, 0, m33, c33));
    REFUSED(gpk_predict_host_multi_cov(h, 3, ptr9, ptr9, n, D, ls9, one9, one9, one9, ptr9, np_, np_, one9, q33, 33, m33, c33));
    REFUSED(gpk_predict_host_multi_cov(h, 9, ptr9, ptr9, n, D, ls9, one9, one9, one9, ptr9, np_, np_, one9, q33, 4, m33, c33));
    REFUSED(gpk_predict_host_multi_cov(h, 3, ptrn, ptr9, n, D, ls9, one9, one9, one9, ptr9, np_, np_, one9, q33, 4, m33, c33));
    REFUSED(gpk_predict_host_multi_cov(h, 3, ptr9, ptr9, n, D, ls9, one9, one9, one9, ptrn, np_, np_, one9, q33, 4, m33, c33));
    REFUSED(gpk_predict_host_multi_cov(h, 3, ptr9, ptr9, n, D, ls9, one9, one9, one9, ptr9, 256, 256, one9, q33, 4, m33, c33));
    (void)hipFree(dbuf);
  }

  double sf2[GPK_MAX_BATCH];
  int info[GPK_MAX_BATCH];
  for (int b = 0; b < B; ++b) sf2[b] = 1.0;
  CHECK_GPK(gpk_fit_batched(h, B, X, N, D, Y, ls, D, sf2, noise, jitter, 0, info));

  CHECK_GPK(gpk_predict_batched_cov(h, Xq, M, mean, cov));
  CHECK_GPK(gpk_predict_batched_cov(h, Xs, Ms, smean, scov));
  EXPECT(symmetric(cov, B, M), "the large route's blocks must be symmetric bit for bit");
  EXPECT(symmetric(scov, B, Ms), "the one-call blocks must be symmetric bit for bit");
  /* a second call returns the same bits */
  CHECK_GPK(gpk_predict_batched_cov(h, Xq, M, again, again + nm));
  CHECK_GPK(gpk_predict_batched_cov(h, Xs, Ms, again + nm + nc, again + nm + nc + sm));
  EXPECT(memcmp(out, again, (size_t)total * sizeof(double)) == 0, "a second call must return the same bits");
  /* the means are those of the existing composite */
  double* pm = (double*)malloc((size_t)nm * sizeof(double));
  CHECK_GPK(gpk_predict_batched(h, Xq, M, pm, NULL, 1));
  double worst = 0.0, scale = 0.0;
  for (long i = 0; i < nm; ++i) {
    if (fabs(pm[i]) > scale) scale = fabs(pm[i]);
    if (fabs(pm[i] - mean[i]) > worst) worst = fabs(pm[i] - mean[i]);
  }
  EXPECT(worst <= 1e-12 * scale, "mean against gpk_predict_batched: %g", worst / scale);
  /* the composite's refusals */
  REFUSED(gpk_predict_batched_cov(h, Xs, 0, smean, scov));
  REFUSED(gpk_predict_batched_cov(h, Xs, 16385, smean, scov));
  REFUSED(gpk_predict_batched_cov(h, NULL, Ms, smean, scov));
  REFUSED(gpk_predict_batched_cov(h, Xs, Ms, smean, NULL));
  double* bad = (double*)malloc((size_t)(Ms * D) * sizeof(double));
  memcpy(bad, Xs, (size_t)(Ms * D) * sizeof(double));
  bad[Ms * D - 1] = NAN;
  REFUSED(gpk_predict_batched_cov(h, bad, Ms, again, again + nm));
  bad[Ms * D - 1] = INFINITY;
  REFUSED(gpk_predict_batched_cov(h, bad, Ms, again, again + nm));

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)total, f) != (size_t)total) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("cov[0][0][0] = %.17g, small cov[0][0][0] = %.17g\nC ABI axis cov: OK\n", cov[0], scov[0]);
  free(bad); free(pm); free(again); free(out); free(buf);
  gpk_destroy(h);
  return 0;
}
