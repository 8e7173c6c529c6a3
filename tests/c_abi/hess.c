/* The composite Hessian call from a plain C caller - no Python, no torch: gpk_fit -> gpk_predict_model_hess on a small
 * deterministic problem that the pytest wrapper (tests/test_gpu_hess_c_abi.py) writes as one flat file of doubles (argv[1]):
 *   [N, D, P, M, ls, noise, jitter] X (N x D) Y (N x P) Xq (M x D)
 * and whose results it reads back from argv[2]:
 *   mean (M x P) dmean (M x P x D) hess (M x P x D x D)     then the same three for the first 7 rows alone
 * to compare them with the Python route (GaussianProcessRegressor.predict_hessian) to 1e-12.  All M rows take the general blocks
 * for the mean and its Jacobian, the 7 rows the small-batch launch.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define CHECK_GPK(x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(h)); return 3; } } while (0)
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 4; } } while (0)

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
  const long N = (long)buf[0], M = (long)buf[3];
  const int D = (int)buf[1], P = (int)buf[2];
  const double ls = buf[4], noise = buf[5], jitter = buf[6];
  const double* X = buf + 7;
  const double* Y = X + N * D;
  const double* Xq = Y + N * P;
  EXPECT((Xq + M * D - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));
  CHECK_GPK(gpk_fit(h, X, N, D, Y, P, &ls, 1, 1.0, noise, jitter, 1));

  const long small = M < 7 ? M : 7;
  const long per = P + P * D + P * D * D, total = (M + small) * per;
  double* out = (double*)malloc((size_t)total * sizeof(double));
  for (long i = 0; i < total; ++i) out[i] = NAN;
  double *mean = out, *dmean = mean + M * P, *hess = dmean + M * P * D;
  double *smean = hess + M * P * D * D, *sdmean = smean + small * P, *shess = sdmean + small * P * D;
  CHECK_GPK(gpk_predict_model_hess(h, Xq, M, mean, dmean, hess));
  CHECK_GPK(gpk_predict_model_hess(h, Xq, small, smean, sdmean, shess));
  /* every block symmetric bit for bit; the two batch sizes agree to rounding */
  double scale = 0.0, worst = 0.0;
  for (long i = 0; i < M * P; ++i)
    for (int d = 0; d < D; ++d)
      for (int e = 0; e < D; ++e) {
        const double v = hess[(i * D + d) * D + e];
        EXPECT(isfinite(v), "hess[%ld][%d][%d] is not finite", i, d, e);
        EXPECT(memcmp(&v, &hess[(i * D + e) * D + d], sizeof v) == 0, "hess[%ld] is not symmetric at (%d, %d)", i, d, e);
        if (fabs(v) > scale) scale = fabs(v);
        if (i < small * P && fabs(v - shess[(i * D + d) * D + e]) > worst) worst = fabs(v - shess[(i * D + d) * D + e]);
      }
  EXPECT(worst <= 1e-11 * scale, "7 rows against all rows: %g", worst / scale);
  /* a null hess is refused */
  EXPECT(gpk_predict_model_hess(h, Xq, M, mean, dmean, NULL) == GPK_BAD_ARG, "a null hess must be refused");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)total, f) != (size_t)total) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("hess[0][0][0][:] =");
  for (int d = 0; d < D; ++d) printf(" %.17g", hess[d]);
  printf("\nC ABI hess: OK\n");
  free(out); free(buf);
  gpk_destroy(h);
  return 0;
}
