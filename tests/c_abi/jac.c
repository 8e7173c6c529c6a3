/* The composite gradient call from a plain C caller - no Python, no torch: gpk_fit -> gpk_predict_model_grad on a small
 * deterministic problem that the pytest wrapper (tests/test_gpu_jac_c_abi.py) writes as one flat file of doubles (argv[1]):
 *   [N, D, P, M, ls, noise, jitter] X (N x D) Y (N x P) Xq (M x D)
 * and whose results it reads back from argv[2]:
 *   mean (M x P) var (M x P) dmean (M x P x D) dvar (M x P x D)      then, mean + Jacobian only: mean (M x P) dmean (M x P x D)
 * to compare them with the Python route (GaussianProcessRegressor.predict_jacobian) to 1e-12.  Both batch sizes of the
 * one-call serving path are driven: the first `small` queries alone (M <= 32: the small-batch launches) and all M.
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

  const long nm = M * P, nj = M * P * D;
  double* out = (double*)malloc((size_t)(2 * nm + 2 * nj + nm + nj) * sizeof(double));
  double *mean = out, *var = mean + nm, *dmean = var + nm, *dvar = dmean + nj, *mean2 = dvar + nj, *dmean2 = mean2 + nm;
  for (long i = 0; i < 3 * nm + 3 * nj; ++i) out[i] = NAN;
  CHECK_GPK(gpk_predict_model_grad(h, Xq, M, mean, var, dmean, dvar, 1));
  CHECK_GPK(gpk_predict_model_grad(h, Xq, M, mean2, NULL, dmean2, NULL, 1));
  /* the small-batch launches on the first rows: the same values as the large route to rounding */
  const long small = M < 25 ? M : 25;
  double* s = (double*)malloc((size_t)(2 * small * P + 2 * small * P * D) * sizeof(double));
  double *smean = s, *svar = smean + small * P, *sdmean = svar + small * P, *sdvar = sdmean + small * P * D;
  CHECK_GPK(gpk_predict_model_grad(h, Xq, small, smean, svar, sdmean, sdvar, 1));
  double scale = 0.0, worst = 0.0, vscale = 0.0, vworst = 0.0;
  for (long i = 0; i < small * P * D; ++i) {
    if (fabs(dmean[i]) > scale) scale = fabs(dmean[i]);
    if (fabs(dmean[i] - sdmean[i]) > worst) worst = fabs(dmean[i] - sdmean[i]);
    if (fabs(dvar[i]) > vscale) vscale = fabs(dvar[i]);
    if (fabs(dvar[i] - sdvar[i]) > vworst) vworst = fabs(dvar[i] - sdvar[i]);
  }
  EXPECT(worst <= 1e-11 * scale && vworst <= 1e-11 * vscale, "small path against the large route: %g %g", worst / scale, vworst / vscale);
  /* both or neither */
  EXPECT(gpk_predict_model_grad(h, Xq, M, mean2, var, dmean2, NULL, 1) == GPK_BAD_ARG, "var without dvar must be refused");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)(3 * nm + 3 * nj), f) != (size_t)(3 * nm + 3 * nj)) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("dmean[0][0][:] =");
  for (int d = 0; d < D; ++d) printf(" %.17g", dmean[d]);
  printf("\ndvar[0][0][:] =");
  for (int d = 0; d < D; ++d) printf(" %.17g", dvar[d]);
  printf("\nC ABI jac: OK\n");
  free(s); free(out); free(buf);
  gpk_destroy(h);
  return 0;
}
