/* The per-axis Hessian composite from a plain C caller - no Python, no torch: gpk_fit_batched -> gpk_predict_batched_hess on the
 * problem the pytest wrapper (tests/test_gpu_axis_hess_c_abi.py) writes as one flat file of doubles (argv[1]):
 *   [N, D, B, M, M_small, jitter] X (N x D) Y (N x B) ls (B x D) noise (B) Xq (M x D)
 * and whose results it reads back from argv[2]:
 *   all M rows (the panel route: the fused launches):     mean (M x B) dmean (M x B x D) hess (M x B x D x D)
 *   the first M_small <= 32 rows (the one-call route):     the same three blocks with M_small rows
 * to compare them with the fixture (tests/golden/hess_ref.npz, case axis) on the scaled inputs.
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
  const long N = (long)buf[0], M = (long)buf[3], Ms = (long)buf[4];
  const int D = (int)buf[1], B = (int)buf[2];
  const double jitter = buf[5];
  const double* X = buf + 6;
  const double* Y = X + N * D;
  const double* ls = Y + N * B;
  const double* noise = ls + B * D;
  const double* Xq = noise + B;
  EXPECT((Xq + M * D - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  EXPECT(B <= GPK_MAX_BATCH && Ms >= 1 && Ms <= 32 && Ms <= M, "B = %d, M_small = %ld", B, Ms);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));
  /* nothing fitted yet: refused */
  double dummy[4];
  EXPECT(gpk_predict_batched_hess(h, Xq, 1, dummy, dummy, dummy) == GPK_BAD_ARG, "a call before gpk_fit_batched must be refused");
  double sf2[GPK_MAX_BATCH];
  int info[GPK_MAX_BATCH];
  for (int b = 0; b < B; ++b) sf2[b] = 1.0;
  CHECK_GPK(gpk_fit_batched(h, B, X, N, D, Y, ls, D, sf2, noise, jitter, 0, info));

  const long per = B + B * D + B * D * D, total = (M + Ms) * per;
  double* out = (double*)malloc((size_t)total * sizeof(double));
  for (long i = 0; i < total; ++i) out[i] = NAN;
  double *mean = out, *dmean = mean + M * B, *hess = dmean + M * B * D;
  double *smean = hess + M * B * D * D, *sdmean = smean + Ms * B, *shess = sdmean + Ms * B * D;
  CHECK_GPK(gpk_predict_batched_hess(h, Xq, M, mean, dmean, hess));
  CHECK_GPK(gpk_predict_batched_hess(h, Xq, Ms, smean, sdmean, shess));
  /* mean and Jacobian are those of the gradient composite, bit for bit */
  double* g = (double*)malloc((size_t)(M * B + M * B * D) * sizeof(double));
  CHECK_GPK(gpk_predict_batched_grad(h, Xq, M, g, NULL, g + M * B, NULL, 1));
  EXPECT(memcmp(g, mean, (size_t)(M * B) * sizeof(double)) == 0, "mean differs from gpk_predict_batched_grad's");
  EXPECT(memcmp(g + M * B, dmean, (size_t)(M * B * D) * sizeof(double)) == 0, "dmean differs from gpk_predict_batched_grad's");
  CHECK_GPK(gpk_predict_batched_grad(h, Xq, Ms, g, NULL, g + Ms * B, NULL, 1));
  EXPECT(memcmp(g, smean, (size_t)(Ms * B) * sizeof(double)) == 0, "mean (small) differs from gpk_predict_batched_grad's");
  EXPECT(memcmp(g + Ms * B, sdmean, (size_t)(Ms * B * D) * sizeof(double)) == 0, "dmean (small) differs");
  /* a null hess is refused */
  EXPECT(gpk_predict_batched_hess(h, Xq, Ms, smean, sdmean, NULL) == GPK_BAD_ARG, "a null hess must be refused");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)total, f) != (size_t)total) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("hess[0][0][0][:] =");
  for (int d = 0; d < D; ++d) printf(" %.17g", hess[d]);
  printf("\nC ABI axis hess: OK\n");
  free(g); free(out); free(buf);
  gpk_destroy(h);
  return 0;
}
