/* Greedy conditional-variance selection of inducing inputs from a plain C caller - no Python, no torch: gpk_sparse_begin ->
 * gpk_sparse_hold -> gpk_sparse_select(X = NULL), on the problem the pytest wrapper (tests/test_gpu_sparse_select_c_abi.py)
 * writes as one flat file of doubles (argv[1]):
 *   [n, D, m_max, sf2] X (n x D) ls (D)
 * and whose results it reads back from argv[2] to compare them with the fixture (tests/golden/sparse_select_ref.npz):
 *   selected  idx (m_max, as doubles)  trace (m_max)  dmax (m_max)
 * Here: a second call gives the same bits, host rows give the bits of the held rows, and the status of every bad call.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define CHECK_GPK(x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(h)); return 3; } } while (0)
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 4; } } while (0)
#define REFUSED(x) do { int r_ = (x); EXPECT(r_ == GPK_BAD_ARG && strlen(gpk_last_error(h)) > 0, "%s -> %d: must be refused with a message", #x, r_); } while (0)

typedef struct { int64_t* idx; double* trace; double* dmax; int64_t selected; } result;

static result fresh(long m) {
  result r;
  r.idx = (int64_t*)malloc((size_t)m * sizeof(int64_t));
  r.trace = (double*)malloc((size_t)m * sizeof(double));
  r.dmax = (double*)malloc((size_t)m * sizeof(double));
  r.selected = -1;
  for (long i = 0; i < m; ++i) { r.idx[i] = -1; r.trace[i] = NAN; r.dmax[i] = NAN; }
  return r;
}

static int same(const result* a, const result* b, long m) {
  return a->selected == b->selected && memcmp(a->idx, b->idx, (size_t)m * sizeof(int64_t)) == 0 &&
         memcmp(a->trace, b->trace, (size_t)m * sizeof(double)) == 0 && memcmp(a->dmax, b->dmax, (size_t)m * sizeof(double)) == 0;
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
  const long n = (long)buf[0], m = (long)buf[2];
  const int D = (int)buf[1];
  const double sf2 = buf[3];
  const double* X = buf + 4;
  const double* ls = X + n * D;
  EXPECT((ls + D - buf) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  EXPECT(m >= 2 && m < n && D >= 1 && D <= 16, "n = %ld, m_max = %ld, D = %d", n, m, D);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(gpk_set_stream(h, GPK_OWN_STREAM));
  if (getenv("GPK_DEBUG_FILL")) CHECK_GPK(gpk_set_option(h, "debug_fill", 1));

  result a = fresh(m), b = fresh(m), c = fresh(m), bad = fresh(m);
  double* Y = (double*)calloc((size_t)n, sizeof(double));
  const double zero = 0.0, one = 1.0;

  /* nothing begun yet */
  REFUSED(gpk_sparse_select(h, X, n, m, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  EXPECT(strstr(gpk_last_error(h), "gpk_sparse_begin") != NULL, "message: %s", gpk_last_error(h));
  /* the object: one inducing input (the selection does not read it), one output */
  CHECK_GPK(gpk_sparse_begin(h, X, 1, D, 1, ls, D, sf2, 0.01, 1e-10, 1e-8, &zero, &one));
  /* no held rows */
  REFUSED(gpk_sparse_select(h, NULL, n, m, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  EXPECT(strstr(gpk_last_error(h), "held rows") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(gpk_sparse_hold(h, X, Y, n));
  /* m_max > n, m_max < 1, a row count that is not the held one, negative thresholds, null outputs */
  REFUSED(gpk_sparse_select(h, NULL, n, n + 1, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_sparse_select(h, X, n, n + 1, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_sparse_select(h, NULL, n, 0, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_sparse_select(h, NULL, n - 1, m, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_sparse_select(h, NULL, n, m, -1.0, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_sparse_select(h, NULL, n, m, 1e-10, -1.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_sparse_select(h, NULL, n, m, 1e-10, 0.0, NULL, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_sparse_select(h, NULL, n, m, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, NULL));
  /* a non-finite row */
  {
    double* nf = (double*)malloc((size_t)(n * D) * sizeof(double));
    memcpy(nf, X, (size_t)(n * D) * sizeof(double));
    nf[n * D - 1] = NAN;
    REFUSED(gpk_sparse_select(h, nf, n, m, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
    EXPECT(strstr(gpk_last_error(h), "NaN or infinity") != NULL, "message: %s", gpk_last_error(h));
    free(nf);
  }
  /* batched mode */
  CHECK_GPK(gpk_batch_begin(h, 2));
  REFUSED(gpk_sparse_select(h, NULL, n, m, 1e-10, 0.0, bad.idx, bad.trace, bad.dmax, &bad.selected));
  EXPECT(strstr(gpk_last_error(h), "batched mode") != NULL, "message: %s", gpk_last_error(h));
  CHECK_GPK(gpk_batch_end(h));
  /* the device-pointer building block refuses before anything is launched: the pointers are never followed */
  REFUSED(gpk_greedy_select(h, X, n, D, ls, D, sf2, n + 1, 1e-10, 0.0, (void*)X, bad.idx, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_greedy_select(h, X, n, 17, ls, 1, sf2, m, 1e-10, 0.0, (void*)X, bad.idx, bad.trace, bad.dmax, &bad.selected));
  REFUSED(gpk_greedy_select(h, X, n, D, ls, D, sf2, m, 1e-10, 0.0, NULL, bad.idx, bad.trace, bad.dmax, &bad.selected));
  EXPECT(gpk_greedy_select_bytes(n, m) >= (size_t)(m + 17) * (size_t)n * sizeof(double) && gpk_greedy_select_bytes(n, 16385) == 0 &&
             gpk_greedy_select_bytes(0, 1) == 0, "work-area sizes");
  /* no refused call wrote anything */
  EXPECT(bad.selected == -1, "a refused call wrote the count");
  for (long i = 0; i < m; ++i) EXPECT(bad.idx[i] == -1 && isnan(bad.trace[i]) && isnan(bad.dmax[i]), "a refused call wrote entry %ld", i);

  /* the held rows, twice, and the same rows from the host */
  CHECK_GPK(gpk_sparse_select(h, NULL, n, m, 1e-10, 0.0, a.idx, a.trace, a.dmax, &a.selected));
  CHECK_GPK(gpk_sparse_select(h, NULL, n, m, 1e-10, 0.0, b.idx, b.trace, b.dmax, &b.selected));
  CHECK_GPK(gpk_sparse_select(h, X, n, m, 1e-10, 0.0, c.idx, c.trace, c.dmax, &c.selected));
  EXPECT(a.selected == m, "selected = %ld of %ld", (long)a.selected, m);
  EXPECT(same(&a, &b, m), "two calls must give the same bits");
  EXPECT(same(&a, &c, m), "host rows must give the bits of the held rows");
  /* the object is untouched: still the statistics of the held rows */
  {
    int64_t rows = -1;
    CHECK_GPK(gpk_sparse_export(h, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &rows, NULL, NULL, NULL, NULL));
    EXPECT(rows == n, "rows = %ld", (long)rows);
  }

  const long total = 1 + 3 * m;
  double* out = (double*)malloc((size_t)total * sizeof(double));
  out[0] = (double)a.selected;
  for (long i = 0; i < m; ++i) { out[1 + i] = (double)a.idx[i]; out[1 + m + i] = a.trace[i]; out[1 + 2 * m + i] = a.dmax[i]; }
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), (size_t)total, f) != (size_t)total) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  printf("trace = %.17g\nC ABI sparse select: OK\n", a.trace[m - 1]);
  free(out); free(Y); free(buf);
  gpk_destroy(h);
  return 0;
}
