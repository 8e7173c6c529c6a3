"""Measurements of greedy conditional-variance selection of the sparse GP's inducing inputs ("choosing Z"):
gpk_greedy_select, SparseGP.from_exact(selection="greedy"), SparseGP.train(select_inducing="greedy").

    python tools/exp_sparse_select.py [--quick] [--only time,csv]

Every step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.

a. time: gpk_greedy_select on device pointers at D = 9 (standard normal rows, ls = 2 .. 2.8), n = 262 144 with m = 256 / 1024 /
   4096 and n = 1000 with m = 512; HIP events around the whole call (m + 2 launches).  Step t reads 8 n t bytes of the panel, the
   whole call 8 n m (m - 1) / 2: the rate over the whole call, and over the LAST QUARTER of the steps - the time of the call with m
   steps minus that of the call with 3 m / 4 steps, against the bytes of those steps - which is what the last step runs at (the
   launches are issued from inside the library, so that no event can be put around one of them).  Both against the rate the Gram
   kernel reaches (5.2 - 5.5 TB/s).  At n = 1000 the panel stays in the caches and the time per launch is the launch-bound floor.
b. csv: tools/exp_sparse_z.py's experiment on tests/golden/csv_170501.npz (output 0, 800 rows to train, 200 held out, m = 128 /
   256 / 512): the rms distance of the sparse mean from the exact model in std(y) and the evaluations of the bound, for a random
   Z and the greedy Z, with the kernel trained, with reselection, and with Z trained as well.
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

from exp_sparse_train import mmm  # noqa: E402

STEP_LIMIT_S = {"time": 420, "csv": 420}
GRAM_TBS = (5.2, 5.5)


def timing(quick):
    import torch
    from exp_sparse import dev_ms
    from unmanned_aerial_vehicles_amd.device import Backend
    D = 9
    be = Backend(0)
    ls = np.ascontiguousarray(2.0 * (1.0 + 0.05 * np.arange(D)))
    lsp = ls.ctypes.data_as(C.POINTER(C.c_double))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    big = 32768 if quick else 262144
    for n, m, reps in ((big, 256, 5), (big, 1024, 3), (big, 4096, 1 if not quick else 2), (1000, 512, 5)):
        X = np.random.default_rng(m).standard_normal((n, D))
        dX = be.upload(X)
        work = torch.empty((be.lib.gpk_greedy_select_bytes(n, m) // 8,), dtype=torch.float64, device=be.device)
        idx = torch.zeros((m,), dtype=torch.int64, device=be.device)
        trace, dmax = torch.zeros((m,), dtype=torch.float64, device=be.device), torch.zeros((m,), dtype=torch.float64, device=be.device)
        sel = torch.zeros((1,), dtype=torch.int64, device=be.device)

        def run(steps):
            be.check(be.lib.gpk_greedy_select(be.h, p(dX), n, D, lsp, D, 1.0, steps, 0.0, 0.0, p(work), p(idx), p(trace), p(dmax), p(sel)))

        with be.lock:
            be.bind_stream()
            run(min(m, 64))          # warm-up: code objects, the work area's pages
            be.sync()
            q = 3 * m // 4
            full = [dev_ms(lambda: run(m)) for _ in range(reps)]
            got = int(sel.cpu()[0])
            tr = float(trace.cpu()[got - 1]) / n
            part = [dev_ms(lambda: run(q)) for _ in range(reps)]
        a, b = float(np.median(full)), float(np.median(part))
        by_all = 8.0 * n * m * (m - 1) / 2
        by_last = by_all - 8.0 * n * q * (q - 1) / 2
        r_all, r_last = by_all / a / 1e9, by_last / (a - b) / 1e9
        print(f"select n = {n:6d} m = {m:4d}: {mmm(full)} ({got} selected, trace / n {tr:.3e}); {1e3 * a / (m + 2):7.2f} us per launch; "
              f"panel reads {by_all / 1e9:8.2f} GB = {r_all:5.2f} TB/s = {r_all / GRAM_TBS[1]:.2f} .. {r_all / GRAM_TBS[0]:.2f} of the Gram's rate; "
              f"last quarter of the steps {a - b:9.3f} ms for {by_last / 1e9:8.2f} GB = {r_last:5.2f} TB/s = "
              f"{r_last / GRAM_TBS[1]:.2f} .. {r_last / GRAM_TBS[0]:.2f} of the Gram's rate; floor of the last step "
              f"{8.0 * n * (m - 1) / GRAM_TBS[1] / 1e6:8.2f} us, measured mean of the last quarter {1e3 * (a - b) / (m - q):8.2f} us at "
              f"t = {(m + q - 1) / 2:.0f}", flush=True)
        del work, dX
        torch.cuda.empty_cache()
    be.lib.gpk_destroy(be.h)


def csv():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, SparseGP, WhiteKernel
    d = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "csv_170501.npz"))
    X, Y = d["X10"], d["Y6"]
    sx = X.std(axis=0)
    X = (X - X.mean(axis=0)) / np.where(sx > 0, sx, 1.0)
    Xt, yt, Xh, yh = X[:800], Y[:800, 0], X[800:], Y[800:, 0]
    kern = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.ones(X.shape[1]), (0.1, 100.0)) + WhiteKernel(0.1, (1e-5, 10.0))
    ex = GaussianProcessRegressor(kernel=kern, alpha=1e-6, normalize_y=True, device=0).fit(Xt, yt)
    em = ex.predict(Xh)
    sd = yt.std()
    print(f"csv: exact fit on 800 rows of csv_170501 (output 0), kernel {ex.kernel_}, LML {ex.log_marginal_likelihood_value_:.3f}, "
          f"rms error on the 200 held-out rows {np.sqrt(np.mean((em - yh) ** 2)) / sd:.3f} std(y)", flush=True)

    def line(m, tag, sp, extra=""):
        sm = sp.predict(Xh)
        print(f"csv m = {m:3d} {tag:<58s}: rms |mean - exact| / std(y) {np.sqrt(np.mean((sm - em) ** 2)) / sd:.2e}  max "
              f"{np.max(np.abs(sm - em)) / sd:.2e}   bound {sp.bound():9.3f}   rms error on the held-out rows "
              f"{np.sqrt(np.mean((sm - yh) ** 2)) / sd:.3f} std(y){extra}", flush=True)

    def trained(m, tag, selection, **kw):
        sp = SparseGP.from_exact(ex, inducing=m, random_state=0, selection=selection)
        n = [0]
        orig = sp.log_bound

        def counted(*a, **k):
            n[0] += 1
            return orig(*a, **k)

        sp.log_bound = counted
        t0 = time.perf_counter()
        sp.train(Xt, yt, **kw)
        dt = time.perf_counter() - t0
        rows = {tuple(x) for x in Xt}
        on = sum(tuple(z) in rows for z in sp.inducing_)
        line(m, tag, sp, f"   {n[0]} evaluations, {1e3 * dt:.0f} ms; {on} of {m} inducing inputs are rows")

    for m in (128, 256, 512):
        for sel in ("random", "greedy"):
            line(m, f"{sel} Z, exact fit's hyper-parameters", SparseGP.from_exact(ex, inducing=m, random_state=0, selection=sel).partial_fit(Xt, yt))
        trained(m, "random Z, kernel trained", "random")
        trained(m, "greedy Z of the exact fit's kernel, kernel trained", "greedy")
        trained(m, "greedy Z reselected, kernel trained, 1 round", "random", select_inducing="greedy", selection_rounds=1)
        trained(m, "greedy Z reselected, kernel trained, 3 rounds", "random", select_inducing="greedy", selection_rounds=3)
        trained(m, "greedy start, kernel and Z trained", "random", select_inducing="greedy", selection_rounds=1, train_inducing=True)
        trained(m, "random start, kernel and Z trained", "random", train_inducing=True)
        # the trace term both selections leave under the exact fit's kernel
        sp = SparseGP.from_exact(ex, inducing=m, random_state=0)
        idx, trace = sp.select_inducing(Xt, m)
        print(f"csv m = {m:3d} tr(Kff - Qff) / n under the exact fit's kernel: greedy {trace[-1] / len(Xt):.4e} after {len(idx)} rows", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rows")
    ap.add_argument("--only", default="time,csv")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    a = ap.parse_args()
    if a.step is None:
        print("# tools/exp_sparse_select.py; fp64", flush=True)
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
    import torch
    print(f"## {a.step} on {torch.cuda.get_device_name(0)}", flush=True)
    {"time": lambda: timing(a.quick), "csv": csv}[a.step]()
    return 0


if __name__ == "__main__":
    sys.exit(main())
