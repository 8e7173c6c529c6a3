/* The per-axis gradient composite from a plain C caller - no Python, no torch: gpk_fit_batched -> gpk_predict_batched_grad on
 * the problem the pytest wrapper (tests/test_gpu_axis_jac_c_abi.py) writes as one flat file of doubles (argv[1]):
 *   [N, D, B, M, M_small, jitter] X (N x D) Y (N x B) ls (B x D) noise (B) Xq (M x D)
 * and whose results it reads back from argv[2]:
 *   all M rows (the panel route):        mean (M x B) var (M x B) dmean (M x B x D) dvar (M x B x D)
 *   the first M_small <= 32 rows (one call, three launches):  the same four blocks with M_small rows
 *   the first M_small rows, mean + Jacobian only (one launch): mean (M_small x B) dmean (M_small x B x D)
 * to compare them with the fixture (tests/golden/axis_jac_ref.npz, case csv) after applying the scalers.
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
  EXPECT(gpk_predict_batched_grad(h, Xq, 1, dummy, NULL, dummy, NULL, 1) == GPK_BAD_ARG, "a call before gpk_fit_batched must be refused");
  double sf2[GPK_MAX_BATCH];
  int info[GPK_MAX_BATCH];
  for (int b = 0; b < B; ++b) sf2[b] = 1.0;
  CHECK_GPK(gpk_fit_batched(h, B, X, N, D, Y, ls, D, sf2, noise, jitter, 0, info));

  const long nm = M * B, nj = M * B * D, sm = Ms * B, sj = Ms * B * D;
  const long total = 2 * nm + 2 * nj + 2 * sm + 2 * sj + sm + sj;
  double* out = (double*)malloc((size_t)total * sizeof(double));
  for (long i = 0; i < total; ++i) out[i] = NAN;
  double *mean = out, *var = mean + nm, *dmean = var + nm, *dvar = dmean + nj;
  double *smean = dvar + nj, *svar = smean + sm, *sdmean = svar + sm, *sdvar = sdmean + sj;
  double *mmean = sdvar + sj, *mdmean = mmean + sm;
  CHECK_GPK(gpk_predict_batched_grad(h, Xq, M, mean, var, dmean, dvar, 1));
  CHECK_GPK(gpk_predict_batched_grad(h, Xq, Ms, smean, svar, sdmean, sdvar, 1));
  CHECK_GPK(gpk_predict_batched_grad(h, Xq, Ms, mmean, NULL, mdmean, NULL, 1));
  /* the means are those of the existing composite */
  double* pm = (double*)malloc((size_t)(2 * nm) * sizeof(double));
  CHECK_GPK(gpk_predict_batched(h, Xq, M, pm, pm + nm, 1));
  double worst = 0.0, scale = 0.0;
  for (long i = 0; i < nm; ++i) {
    if (fabs(pm[i]) > scale) scale = fabs(pm[i]);
    if (fabs(pm[i] - mean[i]) > worst) worst = fabs(pm[i] - mean[i]);
  }
  EXPECT(worst <= 1e-12 * scale, "mean against gpk_predict_batched: %g", worst / scale);
  /* both or neither */
  EXPECT(gpk_predict_batched_grad(h, Xq, Ms, mmean, svar, mdmean, NULL, 1) == GPK_BAD_ARG, "var without dvar must be refused");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)total, f) != (size_t)total) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("dmean[0][0][:] =");
  for (int d = 0; d < D; ++d) printf(" %.17g", dmean[d]);
  printf("\nC ABI axis jac: OK\n");
  free(pm); free(out); free(buf);
  gpk_destroy(h);
  return 0;
}
