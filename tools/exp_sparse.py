"""Measurements of the sparse inducing-point GP.

    python tools/exp_sparse.py [--quick] [--only stats,finalize,serve,accuracy]

1. stats: the statistics pass gpk_sparse_accumulate at D = 9, P = 3, m = 256 / 1024 / 4096, N = 262 144 rows resident in
   HBM: ms, TFLOP/s on N m^2 flops (the lower half of the product G = Kuf Kfu; the launch computes the lower tiles of the
   (mp + 128)-wide product, which is that plus the diagonal tiles' upper halves and the targets' tile row) and the share of
   the 78.6 TF fp64 matrix peak.  Beside it, alternated
   call by call in the same run, the same rows through entries that existed before the pass: per panel (the same panel
   size) gpk_cross_gram_t, the targets copied into the panel's last columns, and ONE gpk_gemm_tiles(lower_only = 1,
   beta = 1) with no k split.  Then the slab count swept (option sparse_slabs) against the built-in rule.
2. finalize: gpk_sparse_finalize at m = 256 / 1024 / 4096, and appending 1000 rows + refinalising at m = 1024 (wall clock
   around calls that end in a synchronisation).
3. serve: one row and the 25-row horizon, mean + variance, on a sparse model with m = 1024 (one output: the two-model call;
   three outputs: the one-model call per inverse factor), beside the exact model's predict at N = 1000 and N = 16 384.
4. accuracy: on tests/golden/csv_170501.npz (800 rows to train, 200 held out, hyper-parameters from the exact fit) the
   sparse model with m = 128 / 256 / 512 against the exact model's mean and std on the held-out rows.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 78.6


def dev_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall_us(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts)), 1e6 * float(np.percentile(ts, 99))


def panel_rows(mp):
    """The built-in panel rule of gpk_sparse.hip (sparse_panel_for)."""
    return int(min(16384, max(1024, (128 << 20) // ((mp + 128) * 8) // 256 * 256)))


def stats(m, N, reps, sweep):
    import torch
    from unmanned_aerial_vehicles_amd import _lib
    from unmanned_aerial_vehicles_amd.device import Backend
    D, P = 9, 3
    be = Backend(0)
    rng = np.random.default_rng(m)
    X, Yn, Z = rng.standard_normal((N, D)), rng.standard_normal((N, P)), rng.standard_normal((m, D))
    ls = np.ascontiguousarray(2.0 * (1.0 + 0.05 * np.arange(D)))
    lsp = ls.ctypes.data_as(C.POINTER(C.c_double))
    dX, dY, dZ = be.upload(X), be.upload(Yn), be.upload(Z)
    mp = (m + 127) // 128 * 128
    nt = mp + 128
    S = torch.zeros((nt, nt), dtype=torch.float64, device=be.device)
    S0 = torch.zeros((nt, nt), dtype=torch.float64, device=be.device)
    panel = panel_rows(mp)
    F = torch.zeros((panel, nt), dtype=torch.float64, device=be.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lib, h = be.lib, be.h

    def new():
        be.check(lib.gpk_sparse_accumulate(h, p(dX), p(dY), N, p(dZ), m, D, P, lsp, 1.0, p(S), nt))

    def old():
        for r0 in range(0, N, panel):
            n = min(panel, N - r0)
            npad = (n + 127) // 128 * 128
            be.check(lib.gpk_cross_gram_t(h, _lib.GPK_F64, p(dX[r0:]), n, p(dZ), m, D, lsp, 1.0, p(F), nt))
            F[:n, mp:mp + P].copy_(dY[r0:r0 + n])
            if npad > n:
                F[n:npad, mp:].zero_()
            be.check(lib.gpk_gemm_tiles(h, _lib.GPK_F64, 1, 1, p(F), nt, p(F), nt, p(S0), nt, nt, nt, npad, 1.0, 1.0, 1))

    with be.lock:
        be.bind_stream()
        new(), old()
        be.sync()
        S.zero_(), S0.zero_()
        new(), old()
        be.sync()
        lo = torch.tril(S0)
        err = float((torch.tril(S) - lo).abs().max() / lo.abs().max())
        tn, to = [], []
        for _ in range(reps):
            tn.append(dev_ms(new))
            to.append(dev_ms(old))
        fl = 1.0 * N * m * m      # the lower half of the product: N m^2 / 2 multiply-adds
        a, b = float(np.median(tn)), float(np.median(to))
        print(f"stats m = {m:5d} N = {N} panel = {panel}: new {a:8.3f} ms [{min(tn):.3f} .. {max(tn):.3f}] = {fl / a / 1e9:5.1f} TF "
              f"({100 * fl / a / 1e9 / PEAK_TF:4.1f} % of the fp64 matrix peak)   cross + one GEMM per panel {b:8.3f} ms "
              f"[{min(to):.3f} .. {max(to):.3f}] = {fl / b / 1e9:5.1f} TF   old / new {b / a:5.2f}   max |new - old| / max |old| "
              f"{err:.1e}", flush=True)
        if sweep:
            line = []
            for s in (1, 2, 4, 8, 16, 32, 0):
                be.set_options(sparse_slabs=s)
                new()
                be.sync()
                line.append(f"{'rule' if s == 0 else s}: {np.median([dev_ms(new) for _ in range(reps)]):.3f}")
            print(f"      m = {m:5d} slabs -> ms   " + "   ".join(line), flush=True)
            line = []
            for rows in (2048, 4096, 8192, 16384, 0):
                be.set_options(sparse_panel=rows)
                new()
                be.sync()
                line.append(f"{'rule' if rows == 0 else rows}: {np.median([dev_ms(new) for _ in range(reps)]):.3f}")
            print(f"      m = {m:5d} panel rows -> ms   " + "   ".join(line), flush=True)
    lib.gpk_destroy(h)
    del S, S0, F, dX, dY, dZ
    torch.cuda.empty_cache()


def sparse_model(m, N, P, D=9, seed=0):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    rng = np.random.default_rng(seed + m)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, P))) + 0.1 * rng.standard_normal((N, P))
    kern = ConstantKernel(1.0) * RBF(2.0 * (1.0 + 0.05 * np.arange(D))) + WhiteKernel(0.01)
    gp = SparseGP(kern, X[:m], alpha=1e-6, jitter_uu=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0), device=0)
    return gp.partial_fit(X, Y if P > 1 else Y[:, 0]), X, Y, rng


def finalize(reps):
    for m in (256, 1024, 4096):
        gp, X, Y, rng = sparse_model(m, 20000, 3)
        be = gp._backend()
        info = C.c_int(0)

        def fin():
            be.check(be.lib.gpk_sparse_finalize(be.h, C.byref(info)))

        t = wall_us(fin, reps, warm=3)
        msg = f"finalize m = {m:5d}: {t[0] / 1e3:8.3f} ms (p99 {t[1] / 1e3:.3f})"
        if m == 1024:
            Xn, Yn = X[:1000], Y[:1000]

            def append():
                gp.partial_fit(Xn, Yn)
                gp._ensure()

            t2 = wall_us(append, reps, warm=3)
            msg += f"   append 1000 rows + refinalise: {t2[0] / 1e3:8.3f} ms (p99 {t2[1] / 1e3:.3f})"
        print(msg, flush=True)
        del gp


def serve(reps):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    D = 9
    for P in (1, 3):
        gp, X, Y, rng = sparse_model(1024, 20000, P)
        for rows in (1, 25):
            Xq = np.ascontiguousarray(rng.standard_normal((rows, D)))
            t = wall_us(lambda: gp.predict(Xq, return_std=True), reps)
            print(f"serve sparse m = 1024, {P} output(s), {rows:2d} row(s): mean + std {t[0]:7.1f} us (p99 {t[1]:7.1f})", flush=True)
        del gp
    for N in (1000, 16384):
        for P in (1, 3):
            rng = np.random.default_rng(N)
            X = rng.standard_normal((N, D))
            Y = np.sin(X @ rng.standard_normal((D, P))) + 0.1 * rng.standard_normal((N, P))
            kern = ConstantKernel(1.0) * RBF(2.0 * (1.0 + 0.05 * np.arange(D))) + WhiteKernel(0.01)
            ex = GaussianProcessRegressor(kernel=kern, alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(
                X, Y if P > 1 else Y[:, 0])
            for rows in (1, 25):
                Xq = np.ascontiguousarray(rng.standard_normal((rows, D)))
                t = wall_us(lambda: ex.predict(Xq, return_std=True), reps)
                print(f"serve exact N = {N:5d}, {P} output(s), {rows:2d} row(s): mean + std {t[0]:7.1f} us (p99 {t[1]:7.1f})",
                      flush=True)
            del ex


def accuracy():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, SparseGP, WhiteKernel
    d = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "csv_170501.npz"))
    X, Y = d["X10"], d["Y6"]
    sx = X.std(axis=0)
    X = (X - X.mean(axis=0)) / np.where(sx > 0, sx, 1.0)
    Xt, yt, Xh = X[:800], Y[:800, 0], X[800:]
    kern = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.ones(X.shape[1]), (0.1, 100.0)) + WhiteKernel(0.1, (1e-5, 10.0))
    ex = GaussianProcessRegressor(kernel=kern, alpha=1e-6, normalize_y=True, device=0).fit(Xt, yt)
    em, es = ex.predict(Xh, return_std=True)
    print(f"accuracy: exact fit on 800 rows of csv_170501 (output 0), kernel {ex.kernel_}, LML {ex.log_marginal_likelihood_value_:.3f}",
          flush=True)
    for m in (128, 256, 512):
        sp = SparseGP.from_exact(ex, inducing=m, random_state=0).partial_fit(Xt, yt)
        sm, ss = sp.predict(Xh, return_std=True)
        print(f"accuracy m = {m:3d}: on the 200 held-out rows  max |mean - exact| / std(y) {np.max(np.abs(sm - em)) / yt.std():.2e}  "
              f"rms {np.sqrt(np.mean((sm - em) ** 2)) / yt.std():.2e}   max |std / exact - 1| {np.max(np.abs(ss / es - 1)):.2e}   "
              f"bound {sp.bound():.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rows and repetitions")
    ap.add_argument("--only", default="stats,finalize,serve,accuracy")
    a = ap.parse_args()
    import torch
    print(f"# tools/exp_sparse.py on {torch.cuda.get_device_name(0)}; fp64", flush=True)
    only = a.only.split(",")
    if "stats" in only:
        for m in (256, 1024, 4096):
            stats(m, 32768 if a.quick else 262144, 3 if a.quick else 7, sweep=True)
    if "finalize" in only:
        finalize(5 if a.quick else 20)
    if "serve" in only:
        serve(200 if a.quick else 1000)
    if "accuracy" in only:
        accuracy()


if __name__ == "__main__":
    main()
