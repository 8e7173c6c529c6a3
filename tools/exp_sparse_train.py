"""Measurements of the sparse GP's training: gpk_sparse_eval, the row pass, SparseGP.train.

    python tools/exp_sparse_train.py [--quick] [--only breakdown,against,unchanged,csv,train]     (GPK_OPTS=sparse_panel=4096,...)

Every step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.

a. breakdown: one gpk_sparse_eval with gradient at D = 9, P = 3, N = 262 144 held rows, m = 256 / 1024 / 4096, alternated
   call by call with the value-only evaluation; min / median / max of the wall clock, and from gpk_timing's brackets the
   statistics pass, the row pass and the Kuu term (gpk_lml_grad's pass).  assembly = value-only evaluation - statistics;
   m x m products (and the small reductions) = the rest.  The row pass's rate on its 2 N nt mp flops (nt = mp + 128) and its
   share of the 78.6 TF fp64 matrix peak.
b. against: gpk_sparse_grad_pass beside the same sums from entries that existed before it, alternated call by call: per
   panel (the same panel size) gpk_cross_gram_t, the targets copied in, ONE gpk_gemm_tiles that stores Q = F C, and a torch
   reduction of Q o Kfu o ((x - z) / ls)^2.
c. unchanged: the statistics pass and gpk_sparse_finalize as tools/exp_sparse.py measures them (the same launches as
   before the training entries existed).
d. csv: on tests/golden/csv_170501.npz (output 0, 800 rows to train, 200 held out) the sparse model with m = 128 / 256 / 512
   against the exact model's mean and std on the held-out rows, with the exact fit's hyper-parameters and after `train`.
e. train: wall clock of SparseGP.train on 262 144 rows at m = 1024 (targets sin(0.25 x.w) + noise: at the frequency of the
   other steps' targets the optimiser's first step lands in the all-noise corner after 10 evaluations), and its number of
   evaluations.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

PEAK_TF = 78.6
STEP_LIMIT_S = {"breakdown": 420, "against": 420, "unchanged": 300, "csv": 240, "train": 300}


def mmm(ts):
    return f"{np.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def problem(m, N, P, D=9, freq=1.0):
    rng = np.random.default_rng(m)
    X = rng.standard_normal((N, D))
    Y = np.sin(freq * (X @ rng.standard_normal((D, P)))) + 0.1 * rng.standard_normal((N, P))
    return X, Y


def model(m, X, Y):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    D = X.shape[1]
    kern = ConstantKernel(1.0) * RBF(2.0 * (1.0 + 0.05 * np.arange(D)), (0.1, 100.0)) + WhiteKernel(0.05, (1e-4, 10.0))
    return SparseGP(kern, X[:m], alpha=1e-6, jitter_uu=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0), device=0)


def breakdown(N, reps):
    from unmanned_aerial_vehicles_amd import _lib
    for m in (256, 1024, 4096):
        X, Y = problem(m, N, 3)
        gp = model(m, X, Y).hold(X, Y)
        be = gp._backend()
        theta = gp.kernel_.theta
        be.check(be.lib.gpk_timing(be.h, 1))
        full, value = [], []
        for i in range(reps + 1):                    # (the first pair warms up: allocations, scratch)
            t0 = time.perf_counter()
            gp.log_bound(theta, eval_gradient=True)
            t1 = time.perf_counter()
            gp.log_bound(theta)
            t2 = time.perf_counter()
            if i:
                full.append(1e3 * (t1 - t0))
                value.append(1e3 * (t2 - t1))

        def times(tag, every):
            ms = np.zeros(64)
            n = C.c_int(0)
            be.check(be.lib.gpk_kernel_times(be.h, tag, ms.ctypes.data_as(_lib._dp), 64, C.byref(n)))
            return list(ms[:n.value][-every * reps:])

        st, rp, ku = times(_lib.GPK_TIMED_SPARSE_STATS, 2), times(_lib.GPK_TIMED_SPARSE_PASS, 1), times(_lib.GPK_TIMED_GRAD, 1)
        mp = (m + 127) // 128 * 128
        fl = 2.0 * N * (mp + 128) * mp
        f, v, s, r, k = (float(np.median(a)) for a in (full, value, st, rp, ku))
        print(f"eval m = {m:5d} N = {N}: with gradient {mmm(full)}   value only {mmm(value)}", flush=True)
        print(f"     m = {m:5d} statistics {mmm(st)}   assembly {v - s:8.3f} ms   m x m products + reductions {f - v - r - k:8.3f} ms   "
              f"row pass {mmm(rp)} = {fl / r / 1e9:5.1f} TF ({100 * fl / r / 1e9 / PEAK_TF:4.1f} % of the fp64 matrix peak)   "
              f"Kuu term {mmm(ku)}", flush=True)
        del gp


def against(N, reps):
    import torch
    from exp_sparse import dev_ms, panel_rows
    from unmanned_aerial_vehicles_amd import _lib
    from unmanned_aerial_vehicles_amd.device import Backend
    D, P = 9, 3
    for m in (256, 1024, 4096):
        be = Backend(0)
        rng = np.random.default_rng(m)
        X, Yn, Z = rng.standard_normal((N, D)), rng.standard_normal((N, P)), rng.standard_normal((m, D))
        ls = np.ascontiguousarray(2.0 * (1.0 + 0.05 * np.arange(D)))
        lsp = ls.ctypes.data_as(C.POINTER(C.c_double))
        mp = (m + 127) // 128 * 128
        nt = mp + 128
        Cm = np.zeros((nt, mp))
        Cm[:m, :m] = rng.standard_normal((m, m))
        Cm[mp:mp + P, :m] = rng.standard_normal((P, m))
        dX, dY, dZ, dC = be.upload(X), be.upload(Yn), be.upload(Z), be.upload(Cm)
        dls = be.upload(ls)
        panel = panel_rows(mp)
        F = torch.zeros((panel, nt), dtype=torch.float64, device=be.device)
        Q = torch.zeros((panel, mp), dtype=torch.float64, device=be.device)
        sums = torch.zeros(17, dtype=torch.float64, device=be.device)
        osum = torch.zeros(17, dtype=torch.float64, device=be.device)
        zs = dZ / dls
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        lib, h = be.lib, be.h

        def new():
            be.check(lib.gpk_sparse_grad_pass(h, p(dX), p(dY), N, p(dZ), m, D, P, lsp, 1.0, p(dC), mp, p(sums)))

        def old():
            osum.zero_()
            for r0 in range(0, N, panel):
                n = min(panel, N - r0)
                npad = (n + 127) // 128 * 128
                be.check(lib.gpk_cross_gram_t(h, _lib.GPK_F64, p(dX[r0:]), n, p(dZ), m, D, lsp, 1.0, p(F), nt))
                F[:n, mp:mp + P].copy_(dY[r0:r0 + n])
                if npad > n:
                    F[n:npad].zero_()
                be.check(lib.gpk_gemm_tiles(h, _lib.GPK_F64, 0, 1, p(F), nt, p(dC), mp, p(Q), mp, npad, mp, nt, 1.0, 0.0, 0))
                T = Q[:n, :m] * F[:n, :m]
                osum[16] += T.sum()
                xs = dX[r0:r0 + n] / dls
                for d in range(D):
                    df = xs[:, d, None] - zs[None, :, d]
                    osum[d] += (T * df * df).sum()

        with be.lock:
            be.bind_stream()
            new(), old()
            be.sync()
            idx = list(range(D)) + [16]
            err = float((sums[idx] - osum[idx]).abs().max() / osum[idx].abs().max())
            tn, to = [], []
            for _ in range(reps):
                tn.append(dev_ms(new))
                to.append(dev_ms(old))
        a, b = float(np.median(tn)), float(np.median(to))
        fl = 2.0 * N * nt * mp
        print(f"row pass m = {m:5d} N = {N} panel = {panel}: new {mmm(tn)} = {fl / a / 1e9:5.1f} TF ({100 * fl / a / 1e9 / PEAK_TF:4.1f} % of "
              f"the fp64 matrix peak)   cross + GEMM that stores Q + torch reduction {mmm(to)}   old / new {b / a:5.2f}   "
              f"max |new - old| / max |old| {err:.1e}", flush=True)
        lib.gpk_destroy(h)
        del F, Q, dX, dY, dZ, dC
        torch.cuda.empty_cache()


def unchanged(N, reps):
    import exp_sparse
    for m in (256, 1024, 4096):
        exp_sparse.stats(m, N, reps, sweep=False)
    exp_sparse.finalize(max(reps, 5))


def csv():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, SparseGP, WhiteKernel
    d = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "csv_170501.npz"))
    X, Y = d["X10"], d["Y6"]
    sx = X.std(axis=0)
    X = (X - X.mean(axis=0)) / np.where(sx > 0, sx, 1.0)
    Xt, yt, Xh, yh = X[:800], Y[:800, 0], X[800:], Y[800:, 0]
    kern = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.ones(X.shape[1]), (0.1, 100.0)) + WhiteKernel(0.1, (1e-5, 10.0))
    ex = GaussianProcessRegressor(kernel=kern, alpha=1e-6, normalize_y=True, device=0).fit(Xt, yt)
    em, es = ex.predict(Xh, return_std=True)
    sd = yt.std()
    print(f"csv: exact fit on 800 rows of csv_170501 (output 0), kernel {ex.kernel_}, LML {ex.log_marginal_likelihood_value_:.3f}, "
          f"rms error on the 200 held-out rows {np.sqrt(np.mean((em - yh) ** 2)) / sd:.3f} std(y)", flush=True)

    def line(tag, sp):
        sm, ss = sp.predict(Xh, return_std=True)
        print(f"csv m = {m:3d} {tag}: max |mean - exact| / std(y) {np.max(np.abs(sm - em)) / sd:.2e}  rms {np.sqrt(np.mean((sm - em) ** 2)) / sd:.2e}"
              f"   max |std / exact - 1| {np.max(np.abs(ss / es - 1)):.2e}   bound {sp.bound():.3f}   rms error on the held-out rows "
              f"{np.sqrt(np.mean((sm - yh) ** 2)) / sd:.3f} std(y)", flush=True)

    for m in (128, 256, 512):
        sp = SparseGP.from_exact(ex, inducing=m, random_state=0).partial_fit(Xt, yt)
        line("exact fit's hyper-parameters", sp)
        n = [0]
        orig = sp.log_bound

        def counted(theta=None, eval_gradient=False):
            n[0] += 1
            return orig(theta, eval_gradient)

        sp.log_bound = counted
        t0 = time.perf_counter()
        sp.train(Xt, yt)
        dt = time.perf_counter() - t0
        line(f"after train ({n[0]} evaluations, {1e3 * dt:.0f} ms)", sp)
        print(f"        trained kernel {sp.kernel_}", flush=True)


def train(N):
    m = 1024
    X, Y = problem(m, N, 3, freq=0.25)       # (smooth enough for 1024 inducing inputs in nine dimensions to explain part of it)
    gp = model(m, X, Y)
    n = [0]
    orig = gp.log_bound

    def counted(theta=None, eval_gradient=False):
        n[0] += 1
        return orig(theta, eval_gradient)

    gp.log_bound = counted
    t0 = time.perf_counter()
    gp.hold(X, Y)
    t1 = time.perf_counter()
    b0 = gp.log_bound(gp.kernel_.theta)
    n[0] = 0
    t2 = time.perf_counter()
    gp.train(X, Y)
    t3 = time.perf_counter()
    print(f"train m = {m} N = {N} D = 9 P = 3: hold (upload + statistics) {t1 - t0:.3f} s; train {t3 - t2:.3f} s wall clock, {n[0]} evaluations "
          f"({1e3 * (t3 - t2) / n[0]:.1f} ms each, the upload and the hold included); bound {b0:.1f} -> {gp.bound_value_:.1f}; kernel {gp.kernel_}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rows and repetitions")
    ap.add_argument("--only", default="breakdown,against,unchanged,csv,train")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    a = ap.parse_args()
    N, reps = (32768, 3) if a.quick else (262144, 5)
    if a.step is None:
        print("# tools/exp_sparse_train.py; fp64; GPK_OPTS = %r" % os.environ.get("GPK_OPTS", ""), flush=True)
        for step in a.only.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--quick"] if a.quick else [])
            try:
                rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
            except subprocess.TimeoutExpired:
                print(f"step {step}: no result within {STEP_LIMIT_S[step]} s - stopping here", flush=True)
                return 124
            if rc != 0:
                print(f"step {step}: exit status {rc} - stopping here", flush=True)
                return rc
        return 0
    import gpk_opts
    gpk_opts.install()      # GPK_OPTS=sparse_panel=4096,...: A/B switches
    import torch
    print(f"## {a.step} on {torch.cuda.get_device_name(0)}", flush=True)
    {"breakdown": lambda: breakdown(N, reps), "against": lambda: against(N, reps), "unchanged": lambda: unchanged(N, reps),
     "csv": csv, "train": lambda: train(N)}[a.step]()
    return 0


if __name__ == "__main__":
    sys.exit(main())
