"""Measurements of training the sparse GP's inducing inputs ("training Z"): the column pass,
gpk_sparse_eval_z, SparseGP.train(train_inducing=True).

    python tools/exp_sparse_z.py [--quick] [--only colpass,eval,csv]     (GPK_OPTS=sparse_panel=4096,...)

Every step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.

a. colpass: gpk_sparse_zgrad_pass at D = 9, P = 3, N = 262 144 rows, m = 256 / 1024 / 4096 (the shapes of
   tools/exp_sparse_train.py) beside the same sums from entries that existed before it, alternated call by call: per panel (the
   same panel size) gpk_cross_gram_t, the targets copied in, ONE gpk_gemm_tiles that stores Q = F C, and a torch reduction of
   Q o Kfu o (x - z) / ls over the panel's rows by exact differences.  Median [min .. max] of five.
b. eval: gpk_sparse_eval_z with gradZ beside gpk_sparse_eval with gradient (the launches profiles/r13_exp_sparse_train.log
   measured) and the value alone, alternated call by call; from gpk_timing's brackets the two passes over the rows.
c. csv: tools/exp_sparse_train.py's experiment on tests/golden/csv_170501.npz (output 0, 800 rows to train, 200 held out, m =
   128 / 256 / 512) with a third column: after train(train_inducing=True).
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

from exp_sparse_train import PEAK_TF, mmm, model, problem  # noqa: E402

STEP_LIMIT_S = {"colpass": 420, "eval": 420, "csv": 300}


def colpass(N, reps):
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
        R = torch.zeros((mp, 17), dtype=torch.float64, device=be.device)
        oR = torch.zeros((mp, 17), dtype=torch.float64, device=be.device)
        zs = dZ / dls
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        lib, h = be.lib, be.h

        def new():
            be.check(lib.gpk_sparse_zgrad_pass(h, p(dX), p(dY), N, p(dZ), m, D, P, lsp, 1.0, p(dC), mp, p(R)))

        def old():
            oR.zero_()
            for r0 in range(0, N, panel):
                n = min(panel, N - r0)
                npad = (n + 127) // 128 * 128
                be.check(lib.gpk_cross_gram_t(h, _lib.GPK_F64, p(dX[r0:]), n, p(dZ), m, D, lsp, 1.0, p(F), nt))
                F[:n, mp:mp + P].copy_(dY[r0:r0 + n])
                if npad > n:
                    F[n:npad].zero_()
                be.check(lib.gpk_gemm_tiles(h, _lib.GPK_F64, 0, 1, p(F), nt, p(dC), mp, p(Q), mp, npad, mp, nt, 1.0, 0.0, 0))
                T = Q[:n, :m] * F[:n, :m]
                oR[:m, 16] += T.sum(dim=0)
                xs = dX[r0:r0 + n] / dls
                for d in range(D):
                    oR[:m, d] += (T * (xs[:, d, None] - zs[None, :, d])).sum(dim=0)

        with be.lock:
            be.bind_stream()
            new(), old()
            be.sync()
            err = float((R - oR).abs().max() / oR.abs().max())
            tn, to = [], []
            for _ in range(reps):
                tn.append(dev_ms(new))
                to.append(dev_ms(old))
        a, b = float(np.median(tn)), float(np.median(to))
        fl = 2.0 * N * nt * mp
        print(f"column pass m = {m:5d} N = {N} panel = {panel}: new {mmm(tn)} = {fl / a / 1e9:5.1f} TF ({100 * fl / a / 1e9 / PEAK_TF:4.1f} % of "
              f"the fp64 matrix peak)   cross + GEMM that stores Q + torch reduction {mmm(to)}   old / new {b / a:5.2f}   "
              f"max |new - old| / max |old| {err:.1e}", flush=True)
        lib.gpk_destroy(h)
        del F, Q, dX, dY, dZ, dC
        torch.cuda.empty_cache()


def evaluation(N, reps):
    from unmanned_aerial_vehicles_amd import _lib
    for m in (256, 1024, 4096):
        X, Y = problem(m, N, 3)
        gp = model(m, X, Y).hold(X, Y)
        be = gp._backend()
        theta = gp.kernel_.theta
        be.check(be.lib.gpk_timing(be.h, 1))
        withz, full, value, passes = [], [], [], []

        def last_passes():                           # (the ring of brackets holds a few evaluations: read it round by round)
            ms = np.zeros(64)
            n = C.c_int(0)
            be.check(be.lib.gpk_kernel_times(be.h, _lib.GPK_TIMED_SPARSE_PASS, ms.ctypes.data_as(_lib._dp), 64, C.byref(n)))
            return list(ms[:n.value][-3:])           # row pass, column pass (with gradZ); row pass (without)

        for i in range(reps + 1):                    # (the first round warms up: allocations, scratch)
            t0 = time.perf_counter()
            gp.log_bound(theta, eval_gradient=True, eval_inducing_gradient=True)
            t1 = time.perf_counter()
            gp.log_bound(theta, eval_gradient=True)
            t2 = time.perf_counter()
            gp.log_bound(theta)
            t3 = time.perf_counter()
            if i:
                withz.append(1e3 * (t1 - t0))
                full.append(1e3 * (t2 - t1))
                value.append(1e3 * (t3 - t2))
                passes.append(last_passes())
        passes = np.array(passes)
        print(f"eval m = {m:5d} N = {N}: with gradient and gradZ {mmm(withz)}   with gradient {mmm(full)}   value only {mmm(value)}", flush=True)
        print(f"     m = {m:5d} row pass {mmm(list(passes[:, 2]))}   beside gradZ: row pass {mmm(list(passes[:, 0]))}   column pass "
              f"{mmm(list(passes[:, 1]))}   the rest of gradZ (mirror, Kuu kernel, copies) "
              f"{np.median(withz) - np.median(full) - np.median(passes[:, 1]):8.3f} ms", flush=True)
        del gp


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

    def line(m, tag, sp):
        sm, ss = sp.predict(Xh, return_std=True)
        print(f"csv m = {m:3d} {tag}: max |mean - exact| / std(y) {np.max(np.abs(sm - em)) / sd:.2e}  rms {np.sqrt(np.mean((sm - em) ** 2)) / sd:.2e}"
              f"   max |std / exact - 1| {np.max(np.abs(ss / es - 1)):.2e}   bound {sp.bound():.3f}   rms error on the held-out rows "
              f"{np.sqrt(np.mean((sm - yh) ** 2)) / sd:.3f} std(y)", flush=True)

    def trained(m, with_z):
        sp = SparseGP.from_exact(ex, inducing=m, random_state=0)
        n = [0]
        orig = sp.log_bound

        def counted(*a, **k):
            n[0] += 1
            return orig(*a, **k)

        sp.log_bound = counted
        t0 = time.perf_counter()
        sp.train(Xt, yt, train_inducing=with_z)
        dt = time.perf_counter() - t0
        line(m, f"after train{' with Z' if with_z else ''} ({n[0]} evaluations, {1e3 * dt:.0f} ms)", sp)
        print(f"        trained kernel {sp.kernel_}", flush=True)

    for m in (128, 256, 512):
        line(m, "exact fit's hyper-parameters", SparseGP.from_exact(ex, inducing=m, random_state=0).partial_fit(Xt, yt))
        trained(m, False)
        trained(m, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rows and repetitions")
    ap.add_argument("--only", default="colpass,eval,csv")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    a = ap.parse_args()
    N, reps = (32768, 3) if a.quick else (262144, 5)
    if a.step is None:
        print("# tools/exp_sparse_z.py; fp64; GPK_OPTS = %r" % os.environ.get("GPK_OPTS", ""), flush=True)
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
    {"colpass": lambda: colpass(N, reps), "eval": lambda: evaluation(N, reps), "csv": csv}[a.step]()
    return 0


if __name__ == "__main__":
    sys.exit(main())
