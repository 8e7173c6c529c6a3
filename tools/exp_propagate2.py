"""Timings of the second-order horizon propagation (K11, order = 2: the mean takes tr(H Sigma) / 2 per stage, one call per horizon)
in one process on one build.

    python tools/exp_propagate2.py [--quick] [--log profiles/r25_exp_propagate2.log]          (GPK_OPTS=small_path=0,...)
    python tools/exp_propagate2.py --horizons 2 [--only "exact one:4096"]          (no timing: order-2 chains, for a kernel trace)

The configurations of tools/exp_propagate.py and tools/exp_sparse_propagate.py: D = 10, nx = 6, H = 25, R = 1 and 32 rollouts; one
model with P = 6 outputs and six single-output models; exact models at N = 1000 and 4096, sparse models at m = 1024.  Per
configuration, wall time per horizon through the public `propagate`, median of the repetitions after 20 warm-up calls:

  (a)  order = 2 as ONE call (4 H launches, one synchronisation) against the host loop it replaces (`route="host"`: per stage
       `predict_jacobian(return_var=True)` + `predict_hessian` - 2 H calls, 2 H synchronisations, an R x NO x D x D Hessian per
       stage - with NumPy between them).  The condition, as for K11: the one call is not slower in any configuration; the last
       line says whether it held.
  (b)  the order = 2 chain against the order = 1 chain: the ratio, and their difference per stage - the trace launch plus the
       advance launch's share sums.  At the largest exact shape also that per-stage cost against the fp64 vector-issue floor of
       the trace launch's R N (nx (nx + 1) / 2 + D + P) fused multiply-adds on the whole device (256 CUs x 64 lanes, 2.4 GHz);
       the launch itself occupies at most 64 workgroups per model.

The two routes of (a) are compared at 1e-10 of the largest component before anything is timed.  The lines are printed and appended
to --log."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

D, NX, H = 10, 6, 25
FMA_PER_S = 256 * 64 * 2.4e9

ratios = []


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
    G = rng.standard_normal((NX, NX))
    S0 = 1e-3 * (G @ G.T + NX * np.eye(NX))
    return (np.ascontiguousarray(0.3 * rng.standard_normal((R, NX))), np.ascontiguousarray(0.3 * rng.standard_normal((R, H, D - NX))),
            0.5 * (S0 + S0.T))


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def measure(say, tag, model, chain, rows, lin, rng, reps, floor_rows=None):
    """chain: the route that is the one call ("auto" for the exact classes, "chain" for the sparse ones); rows: N or m"""
    for R in (1, 32):
        x0, U, S0 = horizon(rng, R)
        kw = dict(Sigma0=S0, var_includes_noise=True)
        a = model.propagate(x0, U, lin, route=chain, order=2, return_stages=True, **kw)
        b = model.propagate(x0, U, lin, route="host", order=2, return_stages=True, **kw)
        agree = max(relerr(b[0], a[0]), relerr(b[1], a[1]), relerr(b[2]["corr"], a[2]["corr"]))
        assert agree < 1e-10, agree
        t2 = wall_us(lambda: model.propagate(x0, U, lin, route=chain, order=2, **kw), reps)
        tl = wall_us(lambda: model.propagate(x0, U, lin, route="host", order=2, **kw), reps)
        t1 = wall_us(lambda: model.propagate(x0, U, lin, route=chain, **kw), reps)
        per_stage = (t2[0] - t1[0]) / H
        ratios.append((f"{tag}, R = {R}", tl[0] / t2[0]))
        line = (f"{tag}, R = {R:2d}, H = {H}: (a) order 2 one call {t2[0]:8.1f} us (p99 {t2[1]:8.1f})   host loop {tl[0]:8.1f} us "
                f"(p99 {tl[1]:8.1f})   loop / one call {tl[0] / t2[0]:5.2f}   (b) order 1 one call {t1[0]:8.1f} us   order 2 / order 1 "
                f"{t2[0] / t1[0]:5.2f}   the fourth launch {per_stage:5.2f} us per stage   routes agree to {agree:.1e}")
        if floor_rows is not None and R == 32:
            fma = R * floor_rows * (NX * (NX + 1) // 2 + D + NX)      # (P = 6 outputs)
            floor_us = 1e6 * fma / FMA_PER_S
            line += f"   trace launch: {fma} fma, whole-device floor {floor_us:5.2f} us, {100.0 * floor_us / per_stage:4.1f} % of its stage cost"
        say(line)


def build(kind, rows):
    """(tag, model, the one-call route, lin, rng) of a configuration"""
    from unmanned_aerial_vehicles_amd import RBF, BatchedSparseGP, ConstantKernel, GaussianProcessRegressor, SparseGP, WhiteKernel
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP

    def axis_kernel(b):
        return ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.roll(np.linspace(1.5, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))

    if kind == "exact one":
        X, Y, lin, rng = problem(rows)
        gp = GaussianProcessRegressor(kernel=RBF(2.0) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X, Y)
        return f"one model P = 6, N = {rows:5d}", gp, "auto", lin, rng
    if kind == "exact six":
        X, Y, lin, rng = problem(rows, 1)
        bg = BatchedARDGP(optimizer=None, device=0)
        for b in range(NX):
            bg.models.append(GaussianProcessRegressor(kernel=axis_kernel(b), alpha=1e-6, normalize_y=True, optimizer=None,
                                                      device=0).fit(X, Y[:, b]))
        return f"six per-axis models, N = {rows:5d}", bg, "auto", lin, rng
    X, Y, lin, rng = problem(max(2 * rows, 2000), 2 if kind == "sparse one" else 3)
    Z = X[rng.permutation(len(X))[:rows]] + 0.05 * rng.standard_normal((rows, D))
    if kind == "sparse one":
        sp = SparseGP(RBF(2.0) + WhiteKernel(0.05), Z, alpha=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0), device=0).fit(X, Y)
        assert sp.propagate_ok()
        return f"one sparse model P = 6, m = {rows:4d}", sp, "chain", lin, rng
    bg = BatchedSparseGP([SparseGP(ConstantKernel(1.0) * RBF(np.roll(np.linspace(1.5, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1)), Z,
                                   alpha=1e-6, y_mean=float(Y[:, b].mean()), y_std=float(Y[:, b].std()), device=0).fit(X, Y[:, b])
                          for b in range(NX)])
    assert bg.propagate_ok()
    return f"six sparse models, m = {rows:4d}", bg, "chain", lin, rng


def trace(horizons, only):
    """order-2 chains only, for a kernel trace: `horizons` of each kind at N = 1000 / m = 1024, R = 32; only = "kind:rows": that one"""
    kinds = (("exact one", 1000), ("exact six", 1000), ("sparse one", 1024), ("sparse six", 1024))
    if only:
        kinds = ((only.split(":")[0], int(only.split(":")[1])),)
    for kind, rows in kinds:
        tag, model, chain, lin, rng = build(kind, rows)
        x0, U, S0 = horizon(rng, 32)
        for _ in range(horizons):
            model.propagate(x0, U, lin, Sigma0=S0, route=chain, order=2)
        print(f"{tag}: {horizons} order-2 chains of H = {H} stages, 4 H = {4 * H} launches each", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 1000 only, no sparse models")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--horizons", type=int, default=0, help="instead of timing: run this many order-2 chains of each kind (for a kernel trace)")
    ap.add_argument("--only", default="", help='with --horizons: one configuration, "exact one|exact six|sparse one|sparse six:rows"')
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "r25_exp_propagate2.log"))
    a = ap.parse_args()
    import gpk_opts
    import torch
    gpk_opts.install()      # GPK_OPTS=small_path=0,...: A/B switches
    if a.horizons:
        trace(a.horizons, a.only)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/exp_propagate2.py on {torch.cuda.get_device_name(0)}; fp64; D = {D}, nx = {NX}, H = {H}; wall time per horizon "
        f"through `propagate`, median of {a.reps} calls after 20 warm-up calls; GPK_OPTS = {os.environ.get('GPK_OPTS', '')!r}")
    configs = [("exact one", 1000), ("exact six", 1000)]
    if not a.quick:
        configs += [("exact one", 4096), ("exact six", 4096), ("sparse one", 1024), ("sparse six", 1024)]
    for kind, rows in configs:
        tag, model, chain, lin, rng = build(kind, rows)
        measure(say, tag, model, chain, rows, lin, rng, a.reps, floor_rows=rows if (kind, rows) == ("exact one", 4096) else None)
    slow = [(t, r) for t, r in ratios if r < 1.0]
    say("# (a) the order-2 one call is not slower than the host loop in any configuration: "
        + ("holds" if not slow else "DOES NOT HOLD: " + ", ".join(f"{t} ({r:.2f})" for t, r in slow)))
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
