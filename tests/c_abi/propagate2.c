/* Second-order horizon propagation (K11, order = 2) from a plain C caller - no Python, no torch: the four entries
 * gpk_propagate2_host, gpk_propagate2_host_multi, gpk_sparse_propagate2 and gpk_sparse_propagate2_multi, each beside its
 * first-order sibling.  The exact model is fitted with the building blocks as in propagate.c, the sparse models with
 * gpk_sparse_begin -> update -> finalize as in sparse_propagate.c.
 * The pytest wrapper (tests/test_gpu_propagate2_c_abi.py) writes the problem as one flat file of doubles, argv[1]:
 *   [ne]  then ne doubles, the exact part - the layout of propagate.c:
 *     [N, D, P, R, H, sf2, noise, alpha]  ls (D)  y_mean (P)  y_std (P)  X (N x D)  Yn (N x P)  YnT (P x N)  x0 (R x P)
 *     U (R x H x (D - P))  lin (P x D)  Sigma0 (P x P)  Q (P x P)  in_shift (D)  in_scale (D)
 *   then the sparse part - the layout of sparse_propagate.c:
 *     [B, n, m, D, R, H, nx]  per model: X (n x D) y (n) Z (m x D) ls (D) [sf2, noise, alpha, jitter_uu, y_mean, y_std]
 *     coord (B)  in_shift (D)  in_scale (D)  out_shift (B)  out_scale (B)
 *     x0 (R x nx)  U (R x H x (D - nx))  lin (nx x D)  Sigma0 (nx x nx)  Q (nx x nx)
 *     x0s (R x 1)  Us (R x H x (D - 1))  lins (1 x D)  Sigma0s (1)  Qs (1)
 * and compares what this program writes to argv[2] with the dense second-order NumPy form - per entry, in the order above,
 * six blocks: traj, Sigma, mean, var, jac, corr (order = 2).
 * The program itself checks for every entry: order = 1 returns the sibling's bits and a zero-filled corr; two order-2 calls
 * repeat their bits; NULL stage outputs and a NULL corr change nothing; Sigma, mean, var and jac of a one-stage horizon have the
 * bits of order 1; order 0 and 3 are GPK_BAD_ARG with the message, and leave the handle serving.
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpk.h"

#define MAXB 8
#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define CHECK_GPK(hh, x) do { int r_ = (x); if (r_ != GPK_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, r_, gpk_last_error(hh)); return 3; } } while (0)
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 4; } } while (0)

static double* to_device(const double* src, size_t n) {
  double* d = NULL;
  if (hipMalloc((void**)&d, sizeof(double) * (n ? n : 1)) != hipSuccess) return NULL;
  if (n && hipMemcpy(d, src, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) return NULL;
  return d;
}

/* the six result blocks of one entry: traj, Sigma, mean, var, jac, corr */
typedef struct { size_t nT, nS, nM, nJ, all; double *t, *s, *m, *v, *j, *c; } Blocks;
static Blocks blocks(double* base, int H, int R, int nx, int NO, int D) {
  Blocks b;
  b.nT = (size_t)(H + 1) * R * nx; b.nS = b.nT * nx; b.nM = (size_t)H * R * NO; b.nJ = b.nM * D;
  b.all = b.nT + b.nS + 3 * b.nM + b.nJ;
  b.t = base; b.s = b.t + b.nT; b.m = b.s + b.nS; b.v = b.m + b.nM; b.j = b.v + b.nM; b.c = b.j + b.nJ;
  return b;
}
static void fill_nan(double* p, size_t n) { for (size_t i = 0; i < n; ++i) p[i] = NAN; }

/* The checks every entry gets.  CALL2(order, H, blocks, with stages, with corr) is the new entry, CALL1(H, blocks) its sibling;
 * `o` receives the order-2 result that goes to the file, `w` is a second work area of the same size. */
#define RUN_ENTRY(hh, name, o, w, Hh, R_, nx_, NO_, D_)                                                                            \
  do {                                                                                                                            \
    fill_nan(o.t, o.all); fill_nan(w.t, w.all);                                                                                   \
    CHECK_GPK(hh, CALL1(Hh, o));                                                                                                  \
    CHECK_GPK(hh, CALL2(1, Hh, w, 1, 1));                                                                                         \
    EXPECT(!memcmp(o.t, w.t, sizeof(double) * (o.all - o.nM)), name ": order = 1 differs from the first-order entry");            \
    for (size_t i = 0; i < w.nM; ++i) EXPECT(w.c[i] == 0.0, name ": order = 1 left corr[%zu] non-zero", i);                       \
    fill_nan(o.t, o.all); fill_nan(w.t, w.all);                                                                                   \
    CHECK_GPK(hh, CALL2(2, Hh, o, 1, 1));                                                                                         \
    for (size_t i = 0; i < o.all; ++i) EXPECT(isfinite(o.t[i]), name ": out[%zu] is not finite", i);                              \
    CHECK_GPK(hh, CALL2(2, Hh, w, 1, 1));                                                                                         \
    EXPECT(!memcmp(o.t, w.t, sizeof(double) * o.all), name ": two order-2 calls differ");                                         \
    fill_nan(w.t, w.nT + w.nS);                                                                                                   \
    CHECK_GPK(hh, CALL2(2, Hh, w, 0, 0));                                                                                         \
    EXPECT(!memcmp(o.t, w.t, sizeof(double) * (o.nT + o.nS)), name ": NULL stage outputs and corr changed traj or Sigma");        \
    for (long k = 0; k < (long)(Hh + 1) * R_; ++k)                                                                                \
      for (int i = 0; i < nx_; ++i)                                                                                               \
        for (int j = 0; j < i; ++j)                                                                                               \
          EXPECT(!memcmp(o.s + k * nx_ * nx_ + i * nx_ + j, o.s + k * nx_ * nx_ + j * nx_ + i, sizeof(double)),                   \
                 name ": Sigma block %ld is not symmetric", k);                                                                   \
    {                                                                                                                             \
      /* one stage: everything but traj[1] has the bits of order 1, and corr is not zero (Sigma0 is SPD) */                        \
      Blocks a1 = blocks(w.t, 1, R_, nx_, NO_, D_), a2 = blocks(w.t + a1.all, 1, R_, nx_, NO_, D_);                                \
      EXPECT(2 * a1.all <= w.all, name ": work area");                                                                            \
      CHECK_GPK(hh, CALL1(1, a1));                                                                                                \
      CHECK_GPK(hh, CALL2(2, 1, a2, 1, 1));                                                                                       \
      EXPECT(!memcmp(a1.s, a2.s, sizeof(double) * (a1.nS + 2 * a1.nM + a1.nJ)), name ": H = 1, Sigma or a stage output differs"); \
      EXPECT(memcmp(a1.t, a2.t, sizeof(double) * a1.nT) != 0, name ": H = 1, the correction did not move traj[1]");               \
      for (size_t i = 0; i < a2.nM; ++i) EXPECT(a2.c[i] != 0.0, name ": H = 1, corr[%zu] is zero", i);                            \
    }                                                                                                                             \
    EXPECT(CALL2(3, Hh, w, 0, 0) == GPK_BAD_ARG, name ": order = 3");                                                             \
    EXPECT(strstr(gpk_last_error(hh), "order must be 1 or 2") != NULL, "message: %s", gpk_last_error(hh));                        \
    EXPECT(CALL2(0, Hh, w, 0, 0) == GPK_BAD_ARG, name ": order = 0");                                                             \
    EXPECT(CALL2(2, 257, w, 0, 0) == GPK_BAD_ARG, name ": H = 257");                                                              \
    EXPECT(strstr(gpk_last_error(hh), "H must be in [1, 256]") != NULL, "message: %s", gpk_last_error(hh));                       \
    fill_nan(w.t, w.all);                                                                                                         \
    CHECK_GPK(hh, CALL2(2, Hh, w, 1, 1));                                                                                         \
    EXPECT(!memcmp(o.t, w.t, sizeof(double) * o.all), name ": the bits changed under the refused calls");                         \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <input file> <output file>\n", argv[0]); return 1; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  double* file = (double*)malloc(bytes);
  if (fread(file, 1, bytes, f) != (size_t)bytes) { fprintf(stderr, "short read\n"); return 1; }
  fclose(f);
  const long ne = (long)file[0];
  const double* buf = file + 1;

  /* ---- the exact part ------------------------------------------------------------------------------------------------------ */
  const long N = (long)buf[0];
  const int D = (int)buf[1], P = (int)buf[2], R = (int)buf[3], H = (int)buf[4];
  const double sf2 = buf[5], noise = buf[6], alpha_j = buf[7];
  const long nu = D - P;
  const double* ls = buf + 8;
  const double *ym = ls + D, *ys = ym + P, *X = ys + P, *Yn = X + N * D, *YnT = Yn + N * P, *x0 = YnT + N * P;
  const double *U = x0 + (long)R * P, *lin = U + (long)R * H * nu, *S0 = lin + P * D, *Q = S0 + P * P, *ish = Q + P * P, *isc = ish + D;
  EXPECT(isc + D - buf == ne && nu >= 1 && P >= 2 && P <= MAXB && H >= 3, "exact part: %ld doubles", ne);

  gpk_handle h = NULL;
  if (gpk_create(&h, 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
  CHECK_GPK(h, gpk_set_stream(h, GPK_OWN_STREAM));
  CHECK_GPK(h, gpk_set_option(h, "debug_fill", 1));
  const int64_t Np = gpk_padded(N);
  double *dX = to_device(X, N * D), *dYn = to_device(Yn, N * P), *dYnT = to_device(YnT, N * P);
  EXPECT(dX && dYn && dYnT, "device allocation");
  double *dK, *dW, *dtr, *dwinv, *dA, *dAT;
  const size_t nK = (size_t)Np * Np, ntr = (size_t)(Np / 2 + 128) * (Np / 2 + 128);
  CHECK_HIP(hipMalloc((void**)&dK, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dW, sizeof(double) * nK));
  CHECK_HIP(hipMalloc((void**)&dtr, sizeof(double) * ntr));
  CHECK_HIP(hipMalloc((void**)&dwinv, sizeof(double) * Np * GPK_TILE));
  CHECK_HIP(hipMalloc((void**)&dA, sizeof(double) * N * P));
  CHECK_HIP(hipMalloc((void**)&dAT, sizeof(double) * N * P));
  CHECK_HIP(hipMemset(dK, 0xFF, sizeof(double) * nK));
  CHECK_HIP(hipMemset(dW, 0xFF, sizeof(double) * nK));
  CHECK_HIP(hipMemset(dtr, 0xFF, sizeof(double) * ntr));
  int info = -1;
  CHECK_GPK(h, gpk_gram(h, GPK_F64, dX, N, D, ls, sf2, noise + alpha_j, dK, Np));
  CHECK_GPK(h, gpk_potrf(h, dK, Np, Np, dwinv, &info));
  EXPECT(info == 0, "potrf info %d", info);
  CHECK_GPK(h, gpk_trtri(h, dK, Np, Np, dwinv, dW, Np, dtr));
  CHECK_GPK(h, gpk_potrs_inv(h, dW, Np, Np, dYn, N, P, dA));
  for (int b = 0; b < P; ++b) CHECK_GPK(h, gpk_potrs_inv(h, dW, Np, Np, dYnT + (long)b * N, N, 1, dAT + (long)b * N));
  CHECK_GPK(h, gpk_synchronize(h));

  /* ---- the sparse part ----------------------------------------------------------------------------------------------------- */
  const double* sb = buf + ne;
  const int B = (int)sb[0], Ds = (int)sb[3], Rs = (int)sb[4], Hs = (int)sb[5], nx = (int)sb[6];
  const long n = (long)sb[1], m = (long)sb[2];
  EXPECT(B >= 2 && B <= MAXB && Ds >= 2 && Ds <= 16 && nx >= B && nx < Ds && Rs >= 1 && Rs <= 32 && Hs >= 3 && Hs <= 256, "sparse header");
  const long per_model = n * Ds + n + m * Ds + Ds + 6, nus = Ds - nx;
  const double* coord_d = sb + 7 + B * per_model;
  const double *sish = coord_d + B, *sisc = sish + Ds, *osh = sisc + Ds, *osc = osh + B, *sx0 = osc + B;
  const double *sU = sx0 + (long)Rs * nx, *slin = sU + (long)Rs * Hs * nus, *sS0 = slin + (long)nx * Ds, *sQ = sS0 + nx * nx, *x0s = sQ + nx * nx;
  const double *Us = x0s + Rs, *lins = Us + (long)Rs * Hs * (Ds - 1), *S0s = lins + Ds, *Qs = S0s + 1;
  EXPECT((Qs + 1 - file) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
  int scoord[MAXB];
  for (int b = 0; b < B; ++b) scoord[b] = (int)coord_d[b];
  gpk_handle hs[MAXB] = {NULL};
  for (int b = 0; b < B; ++b) {
    if (gpk_create(&hs[b], 0) != GPK_OK) { fprintf(stderr, "gpk_create failed\n"); return 1; }
    CHECK_GPK(hs[b], gpk_set_stream(hs[b], GPK_OWN_STREAM));
    CHECK_GPK(hs[b], gpk_set_option(hs[b], "debug_fill", 1));
    const double* Xb = sb + 7 + b * per_model;
    const double *y = Xb + n * Ds, *Z = y + n, *lsb = Z + m * Ds, *hy = lsb + Ds;
    int inf = 0;
    CHECK_GPK(hs[b], gpk_sparse_begin(hs[b], Z, m, Ds, 1, lsb, Ds, hy[0], hy[1], hy[2], hy[3], hy + 4, hy + 5));
    CHECK_GPK(hs[b], gpk_sparse_update(hs[b], Xb, y, n));
    CHECK_GPK(hs[b], gpk_sparse_finalize(hs[b], &inf));
  }
  gpk_handle sh = hs[0];

  /* ---- results: four entries, six blocks each ---------------------------------------------------------------------------------- */
  Blocks e1 = blocks(file, H, R, P, P, D), e3 = blocks(file, Hs, Rs, 1, 1, Ds), e4 = blocks(file, Hs, Rs, nx, B, Ds);      /* (sizes) */
  const size_t total = 2 * e1.all + e3.all + e4.all;
  size_t wmax = e1.all > e4.all ? e1.all : e4.all;
  if (e3.all > wmax) wmax = e3.all;
  double* out = (double*)malloc(sizeof(double) * total);
  double* work = (double*)malloc(sizeof(double) * wmax);
  EXPECT(out && work, "host allocation");
  const double kss = sf2 + noise;

  /* gpk_propagate2_host: the noise level inside kss, as the estimator calls it */
  {
    Blocks o = blocks(out, H, R, P, P, D), w = blocks(work, H, R, P, P, D);
#define CALL1(H_, b) gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H_, \
                                        b.t, b.s, b.m, b.v, b.j)
#define CALL2(ord, H_, b, st, cr) gpk_propagate2_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, \
                                                      1, Q, R, H_, b.t, b.s, (st) ? b.m : NULL, (st) ? b.v : NULL, (st) ? b.j : NULL, ord, \
                                                      (cr) ? b.c : NULL)
    RUN_ENTRY(h, "gpk_propagate2_host", o, w, H, R, P, P, D);
#undef CALL1
#undef CALL2
  }
  /* gpk_propagate2_host_multi: B = P models on coord 0 .. P - 1 behind the input scaler, the noise through var_includes_noise */
  {
    const double *Xs[MAXB], *As[MAXB], *Ws[MAXB];
    double lsB[MAXB * 16], sf2B[MAXB], kssB[MAXB], noiseB[MAXB];
    int coord[MAXB];
    for (int b = 0; b < P; ++b) {
      Xs[b] = dX; As[b] = dAT + (long)b * N; Ws[b] = dW;
      memcpy(lsB + b * D, ls, sizeof(double) * D);
      sf2B[b] = sf2; kssB[b] = sf2; noiseB[b] = noise; coord[b] = b;
    }
    Blocks o = blocks(out + e1.all, H, R, P, P, D), w = blocks(work, H, R, P, P, D);
#define CALL1(H_, b) gpk_propagate_host_multi(h, P, Xs, As, N, D, lsB, sf2B, ym, ys, Ws, Np, Np, kssB, 0.0, 1, noiseB, P, coord, ish, isc, x0, R, U, \
                                              R, lin, S0, 1, Q, R, H_, b.t, b.s, b.m, b.v, b.j)
#define CALL2(ord, H_, b, st, cr) gpk_propagate2_host_multi(h, P, Xs, As, N, D, lsB, sf2B, ym, ys, Ws, Np, Np, kssB, 0.0, 1, noiseB, P, coord, ish, \
                                                            isc, x0, R, U, R, lin, S0, 1, Q, R, H_, b.t, b.s, (st) ? b.m : NULL,             \
                                                            (st) ? b.v : NULL, (st) ? b.j : NULL, ord, (cr) ? b.c : NULL)
    RUN_ENTRY(h, "gpk_propagate2_host_multi", o, w, H, R, P, P, D);
#undef CALL1
#undef CALL2
  }
  /* gpk_sparse_propagate2 on handle 0: a state of one coordinate, D - 1 controls, the noise level included */
  {
    Blocks o = blocks(out + 2 * e1.all, Hs, Rs, 1, 1, Ds), w = blocks(work, Hs, Rs, 1, 1, Ds);
#define CALL1(H_, b) gpk_sparse_propagate(sh, 1, x0s, Rs, Us, Rs, lins, S0s, 1, Qs, Rs, H_, b.t, b.s, b.m, b.v, b.j)
#define CALL2(ord, H_, b, st, cr) gpk_sparse_propagate2(sh, 1, x0s, Rs, Us, Rs, lins, S0s, 1, Qs, Rs, H_, b.t, b.s, (st) ? b.m : NULL,   \
                                                        (st) ? b.v : NULL, (st) ? b.j : NULL, ord, (cr) ? b.c : NULL)
    RUN_ENTRY(sh, "gpk_sparse_propagate2", o, w, Hs, Rs, 1, 1, Ds);
#undef CALL1
#undef CALL2
  }
  /* gpk_sparse_propagate2_multi: latent variances, both scalers */
  {
    Blocks o = blocks(out + 2 * e1.all + e3.all, Hs, Rs, nx, B, Ds), w = blocks(work, Hs, Rs, nx, B, Ds);
#define CALL1(H_, b) gpk_sparse_propagate_multi(sh, B, hs, 0, nx, scoord, sish, sisc, osh, osc, sx0, Rs, sU, Rs, slin, sS0, 1, sQ, Rs, H_, b.t, b.s, \
                                                b.m, b.v, b.j)
#define CALL2(ord, H_, b, st, cr) gpk_sparse_propagate2_multi(sh, B, hs, 0, nx, scoord, sish, sisc, osh, osc, sx0, Rs, sU, Rs, slin, sS0, 1, sQ, Rs, \
                                                              H_, b.t, b.s, (st) ? b.m : NULL, (st) ? b.v : NULL, (st) ? b.j : NULL, ord,     \
                                                              (cr) ? b.c : NULL)
    RUN_ENTRY(sh, "gpk_sparse_propagate2_multi", o, w, Hs, Rs, nx, B, Ds);
#undef CALL1
#undef CALL2
  }
  EXPECT(gpk_propagate2_host(NULL, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, work,
                             work, NULL, NULL, NULL, 2, NULL) == GPK_BAD_ARG, "null handle");
  EXPECT(gpk_sparse_propagate2(NULL, 1, x0s, Rs, Us, Rs, lins, S0s, 1, Qs, Rs, Hs, work, work, NULL, NULL, NULL, 2, NULL) == GPK_BAD_ARG,
         "null handle");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  if (fwrite(out, sizeof(double), total, f) != total) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  hipFree(dX); hipFree(dYn); hipFree(dYnT); hipFree(dK); hipFree(dW); hipFree(dtr); hipFree(dwinv); hipFree(dA); hipFree(dAT);
  gpk_destroy(h);
  for (int b = 0; b < B; ++b) gpk_destroy(hs[b]);
  free(work); free(out); free(file);
  printf("propagate2 from C: OK\n");
  return 0;
}
