"""Measurements of the per-axis batch of sparse GPs ("the per-axis batch").

    python tools/exp_sparse_batch.py [--quick] [--m 256,1024,4096]

Six single-output sparse models, D = 10, each with its own ARD length-scales, noise and inducing inputs, m = 256 / 1024 / 4096,
one row and the 25-row horizon.  Four calls - mean + std, mean + Jacobian, all four gradient results, mean + covariance - each

    from C       ctypes straight on gpk_sparse_predict_multi[_grad|_cov], preallocated buffers
    from Python  BatchedSparseGP.predict / predict_jacobian

against (a) the six single calls the batch call replaces, in the same process and alternated with it call by call - six
gpk_sparse_predict[_grad|_cov] calls on the six handles from C, six `SparseGP` calls from Python - and (b) the exact per-axis
batch (`BatchedARDGP`, six models on N = 1000 shared rows), the analogue README quotes.  Every figure is the median
[min .. max] of wall-clock samples around calls that end in the entry's own synchronisation, after a warm-up.

Condition (the only one): at m = 1024 the batch call is faster than the six single calls, for each of the four calls at 1 and 25
rows, from C and from Python.  The last lines say whether it holds.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, D = 6, 10
CALLS = ("mean + std", "mean + Jacobian", "all four", "mean + cov")


def stats(ts):
    ts = 1e6 * np.asarray(ts)
    return f"{np.median(ts):7.1f} us [{ts.min():7.1f} .. {ts.max():7.1f}]"


def timed(fns, reps, warm=30):
    """Wall-clock samples of each callable, the callables alternated call by call."""
    for _ in range(warm):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            out[k].append(time.perf_counter() - t0)
    return out


def sparse_models(m, N=3000):
    from unmanned_aerial_vehicles_amd import RBF, BatchedSparseGP, ConstantKernel, SparseGP, WhiteKernel
    rng = np.random.default_rng(17 * m)
    X = rng.standard_normal((max(N, m), D))
    Y = np.sin(X @ rng.standard_normal((D, B))) + 0.1 * rng.standard_normal((len(X), B))
    models = []
    for b in range(B):
        kern = ConstantKernel(0.9 + 0.1 * b) * RBF(1.5 * (1.0 + 0.05 * np.arange(D)) * (1.0 + 0.1 * b)) + WhiteKernel(0.02 * (1 + b))
        Z = X[np.sort(rng.permutation(len(X))[:m])]
        gp = SparseGP(kern, Z, alpha=1e-6, jitter_uu=1e-6, y_mean=Y[:, b].mean(), y_std=Y[:, b].std(), device=0)
        models.append(gp.partial_fit(X, Y[:, b]))
    return BatchedSparseGP(models), rng


def exact_batch():
    from unmanned_aerial_vehicles_amd import BatchedARDGP
    rng = np.random.default_rng(5)
    X = rng.standard_normal((1000, D))
    Y = np.sin(X @ rng.standard_normal((D, B))) + 0.1 * rng.standard_normal((1000, B))
    return BatchedARDGP(length_scale=1.5, noise_level=0.05, alpha=1e-6, optimizer=None, device=0).fit(X, Y)


def c_calls(bg, q):
    """(batch callables, six-single-calls callables) on the C ABI for the four calls."""
    from unmanned_aerial_vehicles_amd import _lib
    dp = _lib._dp
    bes, handles = bg._ensure()
    be, lib, M = bes[0], bes[0].lib, q.shape[0]
    p = lambda a: a.ctypes.data_as(dp)      # noqa: E731
    mean, var, dmean, dvar = np.empty((M, B)), np.empty((M, B)), np.empty((M, B, D)), np.empty((M, B, D))
    cov = np.empty((B, M, M))
    qp, pm, pv, pdm, pdv, pc = p(q), p(mean), p(var), p(dmean), p(dvar), p(cov)
    ok = be.check
    batch = [lambda: ok(lib.gpk_sparse_predict_multi(be.h, B, handles, qp, M, pm, pv, 1)),
             lambda: ok(lib.gpk_sparse_predict_multi_grad(be.h, B, handles, qp, M, pm, None, pdm, None, 1)),
             lambda: ok(lib.gpk_sparse_predict_multi_grad(be.h, B, handles, qp, M, pm, pv, pdm, pdv, 1)),
             lambda: ok(lib.gpk_sparse_predict_multi_cov(be.h, B, handles, qp, M, pm, pc))]
    m1, v1, dm1, dv1, c1 = np.empty(M), np.empty(M), np.empty((M, D)), np.empty((M, D)), np.empty((M, M))
    a, b_, c_, d_, e_ = p(m1), p(v1), p(dm1), p(dv1), p(c1)
    hs = [x.h for x in bes]

    def six(fn):
        def run():
            for x, h in zip(bes, hs):
                x.check(fn(h))
        return run

    single = [six(lambda h: lib.gpk_sparse_predict(h, qp, M, a, b_, 1)),
              six(lambda h: lib.gpk_sparse_predict_grad(h, qp, M, a, None, c_, None, 1)),
              six(lambda h: lib.gpk_sparse_predict_grad(h, qp, M, a, b_, c_, d_, 1)),
              six(lambda h: lib.gpk_sparse_predict_cov(h, qp, M, a, e_))]
    return batch, single


def py_calls(bg, q):
    ms = bg.models
    batch = [lambda: bg.predict(q, return_std=True), lambda: bg.predict_jacobian(q),
             lambda: bg.predict_jacobian(q, return_var=True), lambda: bg.predict(q, return_cov=True)]
    single = [lambda: [g.predict(q, return_std=True) for g in ms], lambda: [g.predict_jacobian(q) for g in ms],
              lambda: [g.predict_jacobian(q, return_var=True) for g in ms], lambda: [g.predict(q, return_cov=True) for g in ms]]
    return batch, single


def exact_calls(ex, q):
    py = [lambda: ex.predict(q, return_std=True), lambda: ex.predict_jacobian(q),
          lambda: ex.predict_jacobian(q, return_var=True), lambda: ex.predict(q, return_cov=True)]
    c = [lambda: ex.predict_host(q, True), lambda: ex.predict_host_grad(q, False), lambda: ex.predict_host_grad(q, True),
         lambda: ex.predict_host_cov(q)]
    return c, py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--m", default="256,1024,4096")
    args = ap.parse_args()
    reps = 60 if args.quick else 300
    ex = exact_batch()
    verdict = []
    for m in [int(x) for x in args.m.split(",")]:
        bg, rng = sparse_models(m)
        for rows in (1, 25):
            q = np.ascontiguousarray(1.1 * rng.standard_normal((rows, D)))
            for who, (batch, single), exact in (("C", c_calls(bg, q), exact_calls(ex, q)[0]),
                                                ("Python", py_calls(bg, q), exact_calls(ex, q)[1])):
                for k, name in enumerate(CALLS):
                    tb, ts, te = timed([batch[k], single[k], exact[k]], reps)
                    ratio = np.median(ts) / np.median(tb)
                    apart = max(tb) < min(ts)
                    print(f"m = {m:4d} rows = {rows:2d} from {who:6s} {name:15s}  batch {stats(tb)}   six calls {stats(ts)}   "
                          f"six / batch {ratio:5.2f} ({'ranges apart' if apart else 'ranges overlap'})   "
                          f"exact batch N = 1000 {stats(te)}", flush=True)
                    if m == 1024:
                        verdict.append((who, rows, name, ratio))
        del bg
    if verdict:
        slow = [v for v in verdict if v[3] <= 1.0]
        print(f"condition at m = 1024 (batch faster than six calls, {len(verdict)} cases): "
              f"{'holds' if not slow else 'FAILS for ' + repr(slow)};  six / batch from {min(v[3] for v in verdict):.2f} "
              f"to {max(v[3] for v in verdict):.2f}")


if __name__ == "__main__":
    main()
