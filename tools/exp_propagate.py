"""Timings of the horizon propagation (K11: mean rollout with the linearised state covariance, one call per horizon) against the
host loop it replaces, in the same session on the same build.

    python tools/exp_propagate.py [--quick] [--log profiles/r22_exp_propagate.log]          (GPK_OPTS=small_path=0,...)

D = 10, nx = 6, H = 25, R = 1 and 32 rollouts; one model with P = 6 outputs at N = 1000 and 4096, and six per-axis models
(BatchedARDGP) at the same N.  Per configuration, wall time per horizon, median of the repetitions after warm-up:

  C    the one-call entry (gpk_propagate_host / gpk_propagate_host_multi through its thin ctypes wrapper: 3 H launches, one
       synchronisation) against H calls of gpk_predict_host_grad / gpk_predict_host_multi_grad (3 launches and one
       synchronisation each, the variance gradient computed and dropped) with the NumPy composition between them;
  py   `propagate(...)` against `propagate(..., route="host")`, the same recursion over `predict_jacobian(return_var=True)`;
  adv  the advance launch alone (event bracket GPK_TIMED_PROPAGATE), median over the stages of the timed calls.

The two routes are compared at the project's fp64 bar before anything is timed.  The lines are printed and appended to --log."""
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


def problem(N, seed=0):
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, D))
    Y = 0.05 * np.sin(X @ rng.standard_normal((D, NX))) + 0.01 * rng.standard_normal((N, NX))
    dt = 0.05
    lin = np.zeros((NX, D))
    lin[0:3, 3:6] = dt * np.eye(3)
    lin[3:6, 6:9] = dt * np.eye(3)
    return X, Y, lin, rng


def horizon(rng, R):
    return np.ascontiguousarray(0.3 * rng.standard_normal((R, NX))), np.ascontiguousarray(0.3 * rng.standard_normal((R, H, D - NX)))


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def report(say, tag, one, loop, adv, agree):
    say(f"{tag}: one call {one[0]:8.1f} us (p99 {one[1]:8.1f})   host loop {loop[0]:8.1f} us (p99 {loop[1]:8.1f})   "
        f"loop / one call {loop[0] / one[0]:5.2f}   launches per stage 3 (loop: 3 + a synchronisation)   "
        f"advance launch {1e3 * adv:5.1f} us   routes agree to {agree:.1e}")


def single(say, N, reps):
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel, _lib
    from unmanned_aerial_vehicles_amd import propagate as pg
    X, Y, lin, rng = problem(N)
    gp = GaussianProcessRegressor(kernel=RBF(2.0) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X, Y)
    dev = gp._dev
    ym, ys = gp._y_train_mean, gp._y_train_std
    kss = gp.kernel_.components().sf2 + 0.05
    std2 = ys ** 2
    for R in (1, 32):
        x0, U = horizon(rng, R)

        def one_c():
            return dev.propagate_host(ym, ys, kss, 0.0, False, 0.0, x0, U, lin, None, None, R, H, False)

        def stage(q):
            mean, var, dmean, _ = dev.predict_grad_host(q, ym, ys, kss, 0.0)
            return mean, dmean, np.outer(var, std2)

        def loop_c():
            return pg.host_loop(stage, list(range(NX)), x0, U, lin, None, None, R, H)

        a, b = one_c(), loop_c()
        agree = max(relerr(a[0], b[0]), relerr(a[1], b[1]))
        assert agree < 1e-8, agree
        tc, tl = wall_us(one_c, reps), wall_us(loop_c, reps)
        dev.timing(True)
        for _ in range(3):
            one_c()
        adv = float(np.median(dev.kernel_times(_lib.GPK_TIMED_PROPAGATE)))
        dev.timing(False)
        report(say, f"C   one model P = 6, N = {N:5d}, R = {R:2d}, H = {H}", tc, tl, adv, agree)
        py = wall_us(lambda: gp.propagate(x0, U, lin, var_includes_noise=True), reps)
        pl = wall_us(lambda: gp.propagate(x0, U, lin, var_includes_noise=True, route="host"), reps)
        report(say, f"py  one model P = 6, N = {N:5d}, R = {R:2d}, H = {H}", py, pl, adv, agree)


def axis(say, N, reps):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel, _lib
    from unmanned_aerial_vehicles_amd import propagate as pg
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    X, Y, lin, rng = problem(N, 1)
    bg = BatchedARDGP(optimizer=None, device=0)
    for b in range(NX):
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.roll(np.linspace(1.5, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))
        bg.models.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X, Y[:, b]))
    sv = bg._serve_state(True, any_dtype=True)
    d0, hp = sv["dev0"], _lib.host_ptr
    coord = (C.c_int * NX)(*range(NX))
    for R in (1, 32):
        x0, U = horizon(rng, R)
        traj, Sigma = np.empty((H + 1, R, NX)), np.empty((H + 1, R, NX, NX))

        def one_c():      # the entry itself, as BatchedARDGP.propagate calls it
            d0.be.call("gpk_propagate_host_multi", NX, sv["X"], sv["alpha"], d0.N, d0.D, hp(sv["ls"]), hp(sv["sf2"]), hp(sv["ym"]),
                       hp(sv["ys"]), sv["W"], d0.Np, d0.Np, hp(sv["kss"]), 0.0, 0, None, NX, coord, None, None, hp(x0), R, hp(U), R,
                       hp(lin), None, 1, None, R, H, hp(traj), hp(Sigma), None, None, None)
            return traj, Sigma

        def stage(q):
            mean, dmean, var, _ = bg.predict_host_grad(q, return_var=True)
            return mean, dmean, var

        def loop_c():
            return pg.host_loop(stage, list(range(NX)), x0, U, lin, None, None, R, H)

        a, b = one_c(), loop_c()
        agree = max(relerr(a[0], b[0]), relerr(a[1], b[1]))
        assert agree < 1e-8, agree
        tc, tl = wall_us(one_c, reps), wall_us(loop_c, reps)
        d0.be.call("gpk_timing", 1)
        for _ in range(3):
            one_c()
        adv = float(np.median(d0.kernel_times(_lib.GPK_TIMED_PROPAGATE)))
        d0.be.call("gpk_timing", 0)
        report(say, f"C   six per-axis models, N = {N:5d}, R = {R:2d}, H = {H}", tc, tl, adv, agree)
        py = wall_us(lambda: bg.propagate(x0, U, lin, var_includes_noise=True), reps)
        pl = wall_us(lambda: bg.propagate(x0, U, lin, var_includes_noise=True, route="host"), reps)
        report(say, f"py  six per-axis models, N = {N:5d}, R = {R:2d}, H = {H}", py, pl, adv, agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 1000 only")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "r22_exp_propagate.log"))
    a = ap.parse_args()
    import gpk_opts
    import torch
    gpk_opts.install()      # GPK_OPTS=small_path=0,...: A/B switches
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/exp_propagate.py on {torch.cuda.get_device_name(0)}; fp64; D = {D}, nx = {NX}, H = {H}; wall time per horizon, "
        f"median of {a.reps} calls after 20 warm-up calls; GPK_OPTS = {os.environ.get('GPK_OPTS', '')!r}")
    for N in ((1000,) if a.quick else (1000, 4096)):
        single(say, N, a.reps)
        axis(say, N, a.reps)
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
