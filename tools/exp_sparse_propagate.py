"""Timings of the horizon propagation on the sparse posteriors (K11, the sparse chain: gpk_sparse_propagate[_multi], one call per
horizon) against the host loop it replaces, in the same process on the same build.

    python tools/exp_sparse_propagate.py [--quick] [--log profiles/r23_exp_sparse_propagate.log]     (GPK_OPTS=small_path=0,...)

D = 10, nx = 6, H = 25, R = 1 and 32 rollouts; one sparse model with P = 6 outputs and six single-output sparse models
(BatchedSparseGP) at m = 256, 1024 and 4096 inducing inputs.  Per configuration, wall time per horizon, median of the repetitions
after warm-up:

  C    the one-call entry (gpk_sparse_propagate / gpk_sparse_propagate_multi through its thin ctypes wrapper: 3 H launches, one
       synchronisation) against H calls of gpk_sparse_predict_grad / gpk_sparse_predict_multi_grad (3 launches and one
       synchronisation each, the variance gradient computed and dropped) with the NumPy composition between them;
  py   `propagate(..., route="chain")` against `propagate(..., route="host")`;
  adv  the advance launch alone (event bracket GPK_TIMED_PROPAGATE), median over the stages of the timed calls.

The two routes are compared at the project's fp64 bar before anything is timed, and the agreement is printed.  The acceptance
condition is K11's: the chain is not slower than the loop in any configuration; the last line says whether it held.  The lines are
printed and appended to --log."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

D, NX, H = 10, 6, 25


def wall_us(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts)), 1e6 * float(np.percentile(ts, 99))


def problem(m, seed=0):
    rng = np.random.default_rng(seed + m)
    n = max(2 * m, 2000)
    X = rng.standard_normal((n, D))
    Y = 0.05 * np.sin(X @ rng.standard_normal((D, NX))) + 0.01 * rng.standard_normal((n, NX))
    Z = X[rng.permutation(n)[:m]] + 0.05 * rng.standard_normal((m, D))
    dt = 0.05
    lin = np.zeros((NX, D))
    lin[0:3, 3:6] = dt * np.eye(3)
    lin[3:6, 6:9] = dt * np.eye(3)
    return X, Y, Z, lin, rng


def horizon(rng, R):
    return np.ascontiguousarray(0.3 * rng.standard_normal((R, NX))), np.ascontiguousarray(0.3 * rng.standard_normal((R, H, D - NX)))


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


ratios = []


def report(say, tag, one, loop, adv, agree):
    ratios.append((tag, loop[0] / one[0]))
    say(f"{tag}: chain {one[0]:8.1f} us (p99 {one[1]:8.1f})   host loop {loop[0]:8.1f} us (p99 {loop[1]:8.1f})   "
        f"loop / chain {loop[0] / one[0]:5.2f}   advance launch {1e3 * adv:5.1f} us   routes agree to {agree:.1e}")


def advance_ms(be, call):
    from unmanned_aerial_vehicles_amd import _lib
    be.call("gpk_timing", 1)
    for _ in range(2):
        call()
    ms, n = np.zeros(64), C.c_int(0)
    be.call("gpk_kernel_times", _lib.GPK_TIMED_PROPAGATE, _lib.host_ptr(ms), 64, C.byref(n))
    be.call("gpk_timing", 0)
    return float(np.median(ms[:n.value]))


def single(say, m, reps):
    from unmanned_aerial_vehicles_amd import RBF, SparseGP, WhiteKernel, _lib
    from unmanned_aerial_vehicles_amd import propagate as pg
    X, Y, Z, lin, rng = problem(m)
    sp = SparseGP(RBF(2.0) + WhiteKernel(0.05), Z, alpha=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0), device=0).fit(X, Y)
    sp._ensure()
    assert sp.propagate_ok()
    be, hp = sp._backend(), _lib.host_ptr
    for R in (1, 32):
        x0, U = horizon(rng, R)
        traj, Sigma = np.empty((H + 1, R, NX)), np.empty((H + 1, R, NX, NX))
        mean, var = np.empty((R, NX)), np.empty((R, NX))
        dmean, dvar = np.empty((R, NX, D)), np.empty((R, NX, D))

        def one_c():
            be.call("gpk_sparse_propagate", 1, hp(x0), R, hp(U), R, hp(lin), None, 1, None, R, H, hp(traj), hp(Sigma), None, None, None)
            return traj, Sigma

        def stage(q):
            be.call("gpk_sparse_predict_grad", hp(q), R, hp(mean), hp(var), hp(dmean), hp(dvar), 1)
            return mean, dmean, var

        def loop_c():
            return pg.host_loop(stage, list(range(NX)), x0, U, lin, None, None, R, H)

        a, b = one_c(), loop_c()
        agree = max(relerr(a[0], b[0]), relerr(a[1], b[1]))
        assert agree < 1e-8, agree
        tc, tl = wall_us(one_c, reps), wall_us(loop_c, reps)
        adv = advance_ms(be, one_c)
        report(say, f"C   one model P = 6, m = {m:4d}, R = {R:2d}, H = {H}", tc, tl, adv, agree)
        kw = dict(var_includes_noise=True)
        a, b = sp.propagate(x0, U, lin, route="chain", **kw), sp.propagate(x0, U, lin, route="host", **kw)
        agree = max(relerr(a[0], b[0]), relerr(a[1], b[1]))
        py = wall_us(lambda: sp.propagate(x0, U, lin, route="chain", **kw), reps)
        pl = wall_us(lambda: sp.propagate(x0, U, lin, route="host", **kw), reps)
        report(say, f"py  one model P = 6, m = {m:4d}, R = {R:2d}, H = {H}", py, pl, adv, agree)


def axis(say, m, reps):
    from unmanned_aerial_vehicles_amd import RBF, BatchedSparseGP, ConstantKernel, SparseGP, WhiteKernel, _lib
    from unmanned_aerial_vehicles_amd import propagate as pg
    X, Y, Z, lin, rng = problem(m, 1)
    models = []
    for b in range(NX):
        k = ConstantKernel(1.0) * RBF(np.roll(np.linspace(1.5, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))
        models.append(SparseGP(k, Z, alpha=1e-6, y_mean=float(Y[:, b].mean()), y_std=float(Y[:, b].std()), device=0).fit(X, Y[:, b]))
    bg = BatchedSparseGP(models)
    assert bg.propagate_ok()
    bes, handles = bg._ensure()
    be, hp = bes[0], _lib.host_ptr
    coord = (C.c_int * NX)(*range(NX))
    for R in (1, 32):
        x0, U = horizon(rng, R)
        traj, Sigma = np.empty((H + 1, R, NX)), np.empty((H + 1, R, NX, NX))
        mean, var = np.empty((R, NX)), np.empty((R, NX))
        dmean, dvar = np.empty((R, NX, D)), np.empty((R, NX, D))

        def one_c():      # the entry itself, as BatchedSparseGP.propagate calls it
            be.call("gpk_sparse_propagate_multi", NX, handles, 1, NX, coord, None, None, None, None, hp(x0), R, hp(U), R, hp(lin),
                    None, 1, None, R, H, hp(traj), hp(Sigma), None, None, None)
            return traj, Sigma

        def stage(q):
            be.call("gpk_sparse_predict_multi_grad", NX, handles, hp(q), R, hp(mean), hp(var), hp(dmean), hp(dvar), 1)
            return mean, dmean, var

        def loop_c():
            return pg.host_loop(stage, list(range(NX)), x0, U, lin, None, None, R, H)

        a, b = one_c(), loop_c()
        agree = max(relerr(a[0], b[0]), relerr(a[1], b[1]))
        assert agree < 1e-8, agree
        tc, tl = wall_us(one_c, reps), wall_us(loop_c, reps)
        adv = advance_ms(be, one_c)
        report(say, f"C   six sparse models, m = {m:4d}, R = {R:2d}, H = {H}", tc, tl, adv, agree)
        kw = dict(var_includes_noise=True)
        a, b = bg.propagate(x0, U, lin, route="chain", **kw), bg.propagate(x0, U, lin, route="host", **kw)
        agree = max(relerr(a[0], b[0]), relerr(a[1], b[1]))
        py = wall_us(lambda: bg.propagate(x0, U, lin, route="chain", **kw), reps)
        pl = wall_us(lambda: bg.propagate(x0, U, lin, route="host", **kw), reps)
        report(say, f"py  six sparse models, m = {m:4d}, R = {R:2d}, H = {H}", py, pl, adv, agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="m = 256 only")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--horizons", type=int, default=0, help="instead of timing: run this many chains of each kind at m = 1024 (for a kernel trace)")
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "r23_exp_sparse_propagate.log"))
    a = ap.parse_args()
    import gpk_opts
    import torch
    gpk_opts.install()      # GPK_OPTS=small_path=0,...: A/B switches
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.horizons:
        trace(a.horizons)
        return
    say(f"# tools/exp_sparse_propagate.py on {torch.cuda.get_device_name(0)}; fp64; D = {D}, nx = {NX}, H = {H}; wall time per "
        f"horizon, median of {a.reps} calls after 20 warm-up calls; GPK_OPTS = {os.environ.get('GPK_OPTS', '')!r}")
    for m in ((256,) if a.quick else (256, 1024, 4096)):
        single(say, m, a.reps)
        axis(say, m, a.reps)
    slow = [(t, r) for t, r in ratios if r < 1.0]
    say(f"# condition (the chain is not slower than the loop in any configuration): {'holds' if not slow else 'FAILS for ' + repr(slow)}; "
        f"loop / chain from {min(r for _, r in ratios):.2f} to {max(r for _, r in ratios):.2f}")
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


def trace(count):
    """`count` chains of each kind at m = 1024, R = 32 and nothing else after the set-up: what a kernel trace of the chain is
    taken from (3 H launches per horizon, no small_wtv_grad_kernel)."""
    from unmanned_aerial_vehicles_amd import RBF, BatchedSparseGP, SparseGP, WhiteKernel
    X, Y, Z, lin, rng = problem(1024)
    sp = SparseGP(RBF(2.0) + WhiteKernel(0.05), Z, alpha=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0), device=0).fit(X, Y)
    bg = BatchedSparseGP([SparseGP(RBF(2.0) + WhiteKernel(0.05), Z, alpha=1e-6, device=0).fit(X, Y[:, b]) for b in range(NX)])
    x0, U = horizon(rng, 32)
    for _ in range(count):
        sp.propagate(x0, U, lin, route="chain")
        bg.propagate(x0, U, lin, route="chain")
    print(f"{count} horizons of H = {H} stages on each of one model (P = 6) and six models: {2 * count * H} stages")


if __name__ == "__main__":
    main()
