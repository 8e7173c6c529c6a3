/* Gradient of a horizon cost through the propagation (K11) from a plain C caller - no Python, no torch: the four entries
 * gpk_propagate_grad_host, gpk_propagate_grad_host_multi, gpk_sparse_propagate_grad and gpk_sparse_propagate_grad_multi, each
 * beside its first-order sibling.  The exact model is fitted with the building blocks as in propagate.c, the sparse models with
 * gpk_sparse_begin -> update -> finalize as in sparse_propagate.c.
 * The pytest wrapper (tests/test_gpu_propagate_grad_c_abi.py) writes the problem as one flat file of doubles, argv[1]: the file of
 * propagate2.c -
 *   [ne]  then ne doubles, the exact part:
 *     [N, D, P, R, H, sf2, noise, alpha]  ls (D)  y_mean (P)  y_std (P)  X (N x D)  Yn (N x P)  YnT (P x N)  x0 (R x P)
 *     U (R x H x (D - P))  lin (P x D)  Sigma0 (P x P)  Q (P x P)  in_shift (D)  in_scale (D)
 *   then the sparse part:
 *     [B, n, m, D, R, H, nx]  per model: X (n x D) y (n) Z (m x D) ls (D) [sf2, noise, alpha, jitter_uu, y_mean, y_std]
 *     coord (B)  in_shift (D)  in_scale (D)  out_shift (B)  out_scale (B)
 *     x0 (R x nx)  U (R x H x (D - nx))  lin (nx x D)  Sigma0 (nx x nx)  Q (nx x nx)
 *     x0s (R x 1)  Us (R x H x (D - 1))  lins (1 x D)  Sigma0s (1)  Qs (1)
 * - followed by the seeds: gx, gS of the exact entries ((H + 1) x R x P [x P]), of the sparse batch ((Hs + 1) x Rs x nx [x nx]) and
 * of the single sparse model ((Hs + 1) x Rs x 1 [x 1]).  It compares what this program writes to argv[2] with the dense NumPy
 * adjoint - per entry, in the order above, five blocks: traj, Sigma, dU, dx0, dSigma0.
 * The program itself checks for every entry: traj, Sigma and the stage outputs have the bits of the first-order sibling; two
 * calls repeat their bits; NULL stage outputs, a NULL dSigma0 change nothing else; a NULL gS equals a zero gS; dSigma0 is
 * symmetric bit for bit; a NULL gx, a NULL dx0, a NULL dU, NaN in gx, infinity in gS and H = 257 are GPK_BAD_ARG with a message,
 * leave every output untouched and leave the handle serving.
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

/* the result blocks of one entry: traj, Sigma, dU, dx0, dSigma0 (what goes to the file), then the stage outputs mean, var, jac */
typedef struct { size_t nT, nS, nU, nX, nL, nM, nJ, file, all; double *t, *s, *u, *x, *l, *m, *v, *j; } Blocks;
static Blocks blocks(double* base, int H, int R, int nx, int NO, int D) {
  Blocks b;
  b.nT = (size_t)(H + 1) * R * nx; b.nS = b.nT * nx; b.nU = (size_t)R * H * (D - nx); b.nX = (size_t)R * nx; b.nL = b.nX * nx;
  b.nM = (size_t)H * R * NO; b.nJ = b.nM * D;
  b.file = b.nT + b.nS + b.nU + b.nX + b.nL;
  b.all = b.file + 2 * b.nM + b.nJ;
  b.t = base; b.s = b.t + b.nT; b.u = b.s + b.nS; b.x = b.u + b.nU; b.l = b.x + b.nX; b.m = b.l + b.nL; b.v = b.m + b.nM; b.j = b.v + b.nM;
  return b;
}
static void fill(double* p, size_t n, double v) { for (size_t i = 0; i < n; ++i) p[i] = v; }
static int all_are(const double* p, size_t n, double v) { for (size_t i = 0; i < n; ++i) if (p[i] != v) return 0; return 1; }

/* The checks every entry gets.  CALLG(H, blocks, gx, gS, dU, dx0, dSigma0, with stage outputs) is the new entry, CALL1(H, blocks)
 * its sibling; `o` receives the result that goes to the file, `w` is a second work area of the same size; gx_, gS_: the seeds,
 * bad: a scratch copy of the larger of the two. */
#define RUN_ENTRY(hh, name, o, w, Hh, R_, nx_, gx_, gS_, bad)                                                                      \
  do {                                                                                                                            \
    fill(o.t, o.all, NAN); fill(w.t, w.all, NAN);                                                                                 \
    CHECK_GPK(hh, CALL1(Hh, w));                                                                                                  \
    CHECK_GPK(hh, CALLG(Hh, o, gx_, gS_, o.u, o.x, o.l, 1));                                                                      \
    for (size_t i = 0; i < o.all; ++i) EXPECT(isfinite(o.t[i]), name ": out[%zu] is not finite", i);                              \
    EXPECT(!memcmp(o.t, w.t, sizeof(double) * (o.nT + o.nS)), name ": traj or Sigma differ from the first-order entry");          \
    EXPECT(!memcmp(o.m, w.m, sizeof(double) * (2 * o.nM + o.nJ)), name ": a stage output differs from the first-order entry");    \
    fill(w.t, w.all, NAN);                                                                                                        \
    CHECK_GPK(hh, CALLG(Hh, w, gx_, gS_, w.u, w.x, w.l, 0));                                                                      \
    EXPECT(!memcmp(o.t, w.t, sizeof(double) * o.file), name ": two calls differ, or NULL stage outputs changed a result");        \
    fill(w.t, w.all, NAN);                                                                                                        \
    CHECK_GPK(hh, CALLG(Hh, w, gx_, gS_, w.u, w.x, NULL, 0));                                                                     \
    EXPECT(!memcmp(o.t, w.t, sizeof(double) * (o.file - o.nL)), name ": a NULL dSigma0 changed a result");                        \
    EXPECT(isnan(w.l[0]), name ": a NULL dSigma0 was written");                                                                   \
    for (long k = 0; k < (long)R_; ++k)                                                                                           \
      for (int i = 0; i < nx_; ++i)                                                                                               \
        for (int j = 0; j < i; ++j)                                                                                               \
          EXPECT(!memcmp(o.l + k * nx_ * nx_ + i * nx_ + j, o.l + k * nx_ * nx_ + j * nx_ + i, sizeof(double)),                   \
                 name ": dSigma0 block %ld is not symmetric", k);                                                                 \
    {                                                                                                                             \
      /* a NULL gS is a zero gS, bit for bit */                                                                                   \
      fill(bad, (size_t)(Hh + 1) * R_ * nx_ * nx_, 0.0);                                                                          \
      fill(w.t, w.all, NAN);                                                                                                      \
      CHECK_GPK(hh, CALLG(Hh, w, gx_, bad, w.u, w.x, w.l, 0));                                                                    \
      double* keep = (double*)malloc(sizeof(double) * w.file);                                                                    \
      EXPECT(keep != NULL, "host allocation");                                                                                    \
      memcpy(keep, w.t, sizeof(double) * w.file);                                                                                 \
      fill(w.t, w.all, NAN);                                                                                                      \
      CHECK_GPK(hh, CALLG(Hh, w, gx_, NULL, w.u, w.x, w.l, 0));                                                                   \
      const int same = !memcmp(keep, w.t, sizeof(double) * w.file);                                                               \
      free(keep);                                                                                                                 \
      EXPECT(same, name ": a NULL gS differs from a zero gS");                                                                    \
    }                                                                                                                             \
    /* the refusals: GPK_BAD_ARG, a message, every output untouched */                                                            \
    fill(w.t, w.all, -7.0);                                                                                                       \
    EXPECT(CALLG(Hh, w, NULL, gS_, w.u, w.x, w.l, 1) == GPK_BAD_ARG, name ": NULL gx");                                           \
    EXPECT(strlen(gpk_last_error(hh)) > 0 && strstr(gpk_last_error(hh), "gx") != NULL, "message: %s", gpk_last_error(hh));        \
    EXPECT(CALLG(Hh, w, gx_, gS_, w.u, NULL, w.l, 1) == GPK_BAD_ARG, name ": NULL dx0");                                          \
    EXPECT(strlen(gpk_last_error(hh)) > 0 && strstr(gpk_last_error(hh), "dx0") != NULL, "message: %s", gpk_last_error(hh));       \
    EXPECT(CALLG(Hh, w, gx_, gS_, NULL, w.x, w.l, 1) == GPK_BAD_ARG, name ": NULL dU with controls");                             \
    EXPECT(strlen(gpk_last_error(hh)) > 0 && strstr(gpk_last_error(hh), "dU") != NULL, "message: %s", gpk_last_error(hh));        \
    memcpy(bad, gx_, sizeof(double) * (size_t)(Hh + 1) * R_ * nx_);                                                               \
    bad[(size_t)Hh * R_ * nx_] = NAN;                                                                                             \
    EXPECT(CALLG(Hh, w, bad, gS_, w.u, w.x, w.l, 1) == GPK_BAD_ARG, name ": NaN in gx");                                          \
    EXPECT(strstr(gpk_last_error(hh), "must not contain NaN or infinity") != NULL, "message: %s", gpk_last_error(hh));            \
    memcpy(bad, gS_, sizeof(double) * (size_t)(Hh + 1) * R_ * nx_ * nx_);                                                         \
    bad[1] = INFINITY;                                                                                                            \
    EXPECT(CALLG(Hh, w, gx_, bad, w.u, w.x, w.l, 1) == GPK_BAD_ARG, name ": infinity in gS");                                     \
    EXPECT(strstr(gpk_last_error(hh), "must not contain NaN or infinity") != NULL, "message: %s", gpk_last_error(hh));            \
    EXPECT(CALLG(257, w, gx_, gS_, w.u, w.x, w.l, 1) == GPK_BAD_ARG, name ": H = 257");                                           \
    EXPECT(strstr(gpk_last_error(hh), "H must be in [1, 256]") != NULL, "message: %s", gpk_last_error(hh));                       \
    EXPECT(all_are(w.t, w.all, -7.0), name ": a refused call wrote to an output");                                                \
    fill(w.t, w.all, NAN);                                                                                                        \
    CHECK_GPK(hh, CALLG(Hh, w, gx_, gS_, w.u, w.x, w.l, 1));                                                                      \
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
  /* ---- the seeds ------------------------------------------------------------------------------------------------------------ */
  const double *gxe = Qs + 1, *gSe = gxe + (long)(H + 1) * R * P, *gxb = gSe + (long)(H + 1) * R * P * P;
  const double *gSb = gxb + (long)(Hs + 1) * Rs * nx, *gxs = gSb + (long)(Hs + 1) * Rs * nx * nx, *gSs = gxs + (long)(Hs + 1) * Rs;
  EXPECT((gSs + (long)(Hs + 1) * Rs - file) * (long)sizeof(double) == bytes, "file layout: %ld bytes", bytes);
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

  /* ---- results: four entries, five blocks each go to the file -------------------------------------------------------------------- */
  Blocks e1 = blocks(file, H, R, P, P, D), e3 = blocks(file, Hs, Rs, 1, 1, Ds), e4 = blocks(file, Hs, Rs, nx, B, Ds);      /* (sizes) */
  size_t wmax = e1.all > e4.all ? e1.all : e4.all, smax = (size_t)(H + 1) * R * P * P;
  if (e3.all > wmax) wmax = e3.all;
  if ((size_t)(Hs + 1) * Rs * nx * nx > smax) smax = (size_t)(Hs + 1) * Rs * nx * nx;
  double* out = (double*)malloc(sizeof(double) * wmax * 4);
  double* work = (double*)malloc(sizeof(double) * wmax);
  double* bad = (double*)malloc(sizeof(double) * smax);
  EXPECT(out && work && bad, "host allocation");
  const double kss = sf2 + noise;
  Blocks o1 = blocks(out, H, R, P, P, D), o2 = blocks(out + wmax, H, R, P, P, D), o3 = blocks(out + 2 * wmax, Hs, Rs, 1, 1, Ds);
  Blocks o4 = blocks(out + 3 * wmax, Hs, Rs, nx, B, Ds);

  /* gpk_propagate_grad_host: the noise level inside kss, as the estimator calls it */
  {
    Blocks w = blocks(work, H, R, P, P, D);
#define CALL1(H_, b) gpk_propagate_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H_, \
                                        b.t, b.s, b.m, b.v, b.j)
#define CALLG(H_, b, gx_, gS_, dU_, dx_, dS_, st) gpk_propagate_grad_host(h, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, \
                                                      U, R, lin, S0, 1, Q, R, H_, b.t, b.s, (st) ? b.m : NULL, (st) ? b.v : NULL,         \
                                                      (st) ? b.j : NULL, gx_, gS_, dU_, dx_, dS_)
    RUN_ENTRY(h, "gpk_propagate_grad_host", o1, w, H, R, P, gxe, gSe, bad);
#undef CALL1
#undef CALLG
  }
  /* gpk_propagate_grad_host_multi: B = P models on coord 0 .. P - 1 behind the input scaler, the noise through var_includes_noise */
  {
    const double *Xs[MAXB], *As[MAXB], *Ws[MAXB];
    double lsB[MAXB * 16], sf2B[MAXB], kssB[MAXB], noiseB[MAXB];
    int coord[MAXB];
    for (int b = 0; b < P; ++b) {
      Xs[b] = dX; As[b] = dAT + (long)b * N; Ws[b] = dW;
      memcpy(lsB + b * D, ls, sizeof(double) * D);
      sf2B[b] = sf2; kssB[b] = sf2; noiseB[b] = noise; coord[b] = b;
    }
    Blocks w = blocks(work, H, R, P, P, D);
#define CALL1(H_, b) gpk_propagate_host_multi(h, P, Xs, As, N, D, lsB, sf2B, ym, ys, Ws, Np, Np, kssB, 0.0, 1, noiseB, P, coord, ish, isc, x0, R, U, \
                                              R, lin, S0, 1, Q, R, H_, b.t, b.s, b.m, b.v, b.j)
#define CALLG(H_, b, gx_, gS_, dU_, dx_, dS_, st) gpk_propagate_grad_host_multi(h, P, Xs, As, N, D, lsB, sf2B, ym, ys, Ws, Np, Np, kssB, 0.0, 1,   \
                                                      noiseB, P, coord, ish, isc, x0, R, U, R, lin, S0, 1, Q, R, H_, b.t, b.s,            \
                                                      (st) ? b.m : NULL, (st) ? b.v : NULL, (st) ? b.j : NULL, gx_, gS_, dU_, dx_, dS_)
    RUN_ENTRY(h, "gpk_propagate_grad_host_multi", o2, w, H, R, P, gxe, gSe, bad);
#undef CALL1
#undef CALLG
  }
  /* gpk_sparse_propagate_grad on handle 0: a state of one coordinate, D - 1 controls, the noise level included */
  {
    Blocks w = blocks(work, Hs, Rs, 1, 1, Ds);
#define CALL1(H_, b) gpk_sparse_propagate(sh, 1, x0s, Rs, Us, Rs, lins, S0s, 1, Qs, Rs, H_, b.t, b.s, b.m, b.v, b.j)
#define CALLG(H_, b, gx_, gS_, dU_, dx_, dS_, st) gpk_sparse_propagate_grad(sh, 1, x0s, Rs, Us, Rs, lins, S0s, 1, Qs, Rs, H_, b.t, b.s,             \
                                                      (st) ? b.m : NULL, (st) ? b.v : NULL, (st) ? b.j : NULL, gx_, gS_, dU_, dx_, dS_)
    RUN_ENTRY(sh, "gpk_sparse_propagate_grad", o3, w, Hs, Rs, 1, gxs, gSs, bad);
#undef CALL1
#undef CALLG
  }
  /* gpk_sparse_propagate_grad_multi: latent variances, both scalers */
  {
    Blocks w = blocks(work, Hs, Rs, nx, B, Ds);
#define CALL1(H_, b) gpk_sparse_propagate_multi(sh, B, hs, 0, nx, scoord, sish, sisc, osh, osc, sx0, Rs, sU, Rs, slin, sS0, 1, sQ, Rs, H_, b.t, b.s, \
                                                b.m, b.v, b.j)
#define CALLG(H_, b, gx_, gS_, dU_, dx_, dS_, st) gpk_sparse_propagate_grad_multi(sh, B, hs, 0, nx, scoord, sish, sisc, osh, osc, sx0, Rs, sU, Rs,    \
                                                      slin, sS0, 1, sQ, Rs, H_, b.t, b.s, (st) ? b.m : NULL, (st) ? b.v : NULL,             \
                                                      (st) ? b.j : NULL, gx_, gS_, dU_, dx_, dS_)
    RUN_ENTRY(sh, "gpk_sparse_propagate_grad_multi", o4, w, Hs, Rs, nx, gxb, gSb, bad);
#undef CALL1
#undef CALLG
  }
  EXPECT(gpk_propagate_grad_host(NULL, dX, dA, N, D, P, ls, sf2, ym, ys, dW, Np, Np, kss, 0.0, 0, 0.0, x0, R, U, R, lin, S0, 1, Q, R, H, work,
                                 work, NULL, NULL, NULL, gxe, NULL, work, work, NULL) == GPK_BAD_ARG, "null handle");
  EXPECT(gpk_sparse_propagate_grad(NULL, 1, x0s, Rs, Us, Rs, lins, S0s, 1, Qs, Rs, Hs, work, work, NULL, NULL, NULL, gxs, NULL, work, work,
                                   NULL) == GPK_BAD_ARG, "null handle");

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 1; }
  const Blocks* os[4] = {&o1, &o2, &o3, &o4};
  for (int e = 0; e < 4; ++e)
    if (fwrite(os[e]->t, sizeof(double), os[e]->file, f) != os[e]->file) { fprintf(stderr, "short write\n"); return 1; }
  fclose(f);
  hipFree(dX); hipFree(dYn); hipFree(dYnT); hipFree(dK); hipFree(dW); hipFree(dtr); hipFree(dwinv); hipFree(dA); hipFree(dAT);
  gpk_destroy(h);
  for (int b = 0; b < B; ++b) gpk_destroy(hs[b]);
  free(bad); free(work); free(out); free(file);
  printf("propagate_grad from C: OK\n");
  return 0;
}
