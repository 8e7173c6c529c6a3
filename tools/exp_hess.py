"""Timings of the posterior mean's input Hessian (predict_hessian, K8 second derivatives) against what a caller had before: 2 D
Jacobian calls for a central difference of the Jacobian, on the same build.

    python tools/exp_hess.py [--quick] [--log profiles/r24_exp_hess.log]

1. The control loop, one and 25 rows, D = 10, wall time per call (median and p99):
   one model with P = 6 at N = 1000 and 4096 (gpk_predict_host_hess against 2 D gpk_predict_host_grad calls);
   six per-axis models at N = 1000 and 4096 (gpk_predict_host_multi_hess against 2 D gpk_predict_host_multi_grad calls);
   one sparse model with P = 6 over m = 1024 inducing rows (gpk_sparse_predict_hess against 2 D gpk_sparse_predict_grad calls).
2. Large route, M = 4096 queries at N = 16 384 and 65 536, D = 10, P = 1 and P = 6: gpk_predict_mean_hess against
   gpk_predict_mean_grad on the same queries (CUDA events), with its share of the fp64 vector-issue floor: per (pair, output
   group) D subtracts + D FMAs (distance) + ~20 (exp) and per output 1 + rows of the block (weights) + its triangle entries
   (FMAs), every fp64 vector instruction at the FMA rate.
   The per-axis batch, M = 4096: the fused launch gpk_predict_mean_hess_multi against B gpk_predict_mean_hess launches at
   (N, B, D) = (4096, 6, 10), (16 384, 6, 10), (16 384, 8, 10), (16 384, 6, 16).
3. The worst parity error seen: each timed Hessian against a second-order central difference of the timed Jacobian calls
   (h = 1e-4, its own truncation ~1e-8: a sanity figure, the tests hold the bars), and the large route against the one-call route.
Medians over the repetitions.  The log goes to stdout and, with --log, to that file as well."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VALU_TFLOPS = 78.6      # MI355X fp64 vector peak (FMA = 2 flops)
FD_H = 1e-4

_log = None
_worst = {"fd": 0.0, "route": 0.0}


def say(line):
    print(line, flush=True)
    if _log:
        _log.write(line + "\n")
        _log.flush()


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def wall_us(fn, reps):
    for _ in range(20):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts)), 1e6 * float(np.percentile(ts, 99))


def dev_ms(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def control_loop(name, hess_call, jac_call, Xq, reps):
    """hess_call(X) -> (mean, dmean, hess); jac_call(X) -> dmean.  The baseline: 2 D Jacobian calls, differenced."""
    D = Xq.shape[1]

    def differenced():
        cols = []
        for e in range(D):
            step = np.zeros(D)
            step[e] = FD_H
            cols.append((jac_call(Xq + step) - jac_call(Xq - step)) / (2.0 * FD_H))
        return np.stack(cols, axis=-1)

    hess = hess_call(Xq)[2]
    err = relerr(differenced(), hess)
    _worst["fd"] = max(_worst["fd"], err)
    a = wall_us(lambda: hess_call(Xq), reps)
    b = wall_us(lambda: jac_call(Xq), reps)
    c = wall_us(differenced, max(reps // 10, 20))
    say(f"{name} rows = {len(Xq):2d}: mean+Jacobian+Hessian {a[0]:7.1f} us (p99 {a[1]:7.1f})   one mean+Jacobian call {b[0]:7.1f} us "
        f"(p99 {b[1]:7.1f})   2 D = {2 * D} Jacobian calls {c[0]:8.1f} us: {c[0] / a[0]:5.2f} x the one call   "
        f"Hessian against their difference {err:.1e}")


def flight(N, D=10):
    d = np.load(os.path.join(ROOT, "tests", "golden", "csv_170501.npz"))
    reps = -(-N // len(d["X10"]))
    rng = np.random.default_rng(N)
    X = np.concatenate([d["X10"]] * reps)[:N] + (0.05 * rng.standard_normal((N, D)) if reps > 1 else 0.0)
    Y = np.concatenate([d["Y6"]] * reps)[:N]
    return X, Y, np.ascontiguousarray(d["Xq10"])


def single_model(N, reps):
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    X, Y, Xq = flight(N)
    gp = GaussianProcessRegressor(kernel=RBF(0.5) + WhiteKernel(0.1), alpha=1e-4, normalize_y=True, optimizer=None,
                                  device=0).fit(X, Y)
    for M in (1, 25):
        control_loop(f"one model P = 6, N = {N}", gp.predict_hessian, lambda Z: gp.predict_jacobian(Z)[1], Xq[:M], reps)


def axis_batch(N, B=6, D=10):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, B))) + 0.1 * rng.standard_normal((N, B))
    bg = BatchedARDGP(optimizer=None, device=0)
    for b in range(B):
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.roll(np.linspace(1.2, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))
        bg.models.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=False, optimizer=None, device=0).fit(X, Y[:, b]))
    return bg, rng


def axis_models(N, reps, D=10):
    bg, rng = axis_batch(N)
    Xq = np.ascontiguousarray(rng.standard_normal((25, D)))
    assert bg.predict_host_hess(Xq) is not None
    for M in (1, 25):
        control_loop(f"six per-axis models, N = {N}", bg.predict_hessian, lambda Z: bg.predict_jacobian(Z)[1], Xq[:M], reps)


def axis_large(N, M, reps, B=6, D=10):
    """The fused launch (gpk_predict_mean_hess_multi, through BatchedARDGP's large route) against B gpk_predict_mean_hess launches."""
    import torch
    from unmanned_aerial_vehicles_amd.device import _hp, _p, get_backend
    bg, rng = axis_batch(N, B, D)
    for m in bg.models:
        m._ensure_device()
    f = bg._fused64()
    be = get_backend(0)
    q = be.upload(np.ascontiguousarray(rng.standard_normal((M, D))), torch.float64)
    hess = be.empty((M, B, D, D), torch.float64)

    def fused():
        be.call("gpk_predict_mean_hess_multi", _p(f["X"]), _p(f["alpha"]), f["N"], D, B, _hp(f["ls"]), _hp(f["sf2"]), _hp(f["ys"]),
                _p(q), M, _p(hess))

    def each():
        for m in bg.models:
            m._dev.predict_mean_hess_dev(q, m._y_train_std)

    dev_ms(fused, 2)
    dev_ms(each, 2)
    t_f, t_e = dev_ms(fused, reps), dev_ms(each, reps)
    single = np.stack([m._dev.predict_mean_hess_dev(q[:256], m._y_train_std).cpu().numpy()[:, 0] for m in bg.models], axis=1)
    fused()
    _worst["route"] = max(_worst["route"], relerr(hess[:256].cpu().numpy(), single))
    say(f"per-axis B = {B}, D = {D}, N = {N:6d} M = {M}: predict_mean_hess_multi {t_f:8.3f} ms   {B} predict_mean_hess launches "
        f"{t_e:8.3f} ms ({t_e / t_f:5.2f} x)")
    del bg
    torch.cuda.empty_cache()


def sparse_model(m, reps, n=8192, D=10, P=6):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    rng = np.random.default_rng(m)
    X = rng.standard_normal((n, D))
    Y = 0.3 * np.sin(X @ rng.standard_normal((D, P))) + 0.02 * rng.standard_normal((n, P))
    kern = ConstantKernel(1.0) * RBF(2.0 * np.ones(D)) + WhiteKernel(0.01)
    sp = SparseGP(kern, X[:m], alpha=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0)).fit(X, Y)
    Xq = np.ascontiguousarray(rng.standard_normal((25, D)))
    for M in (1, 25):
        control_loop(f"sparse model P = {P}, m = {m} (n = {n})", sp.predict_hessian, lambda Z: sp.predict_jacobian(Z)[1], Xq[:M], reps)


def large(N, M, P, reps, D=10):
    import torch
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    rng = np.random.default_rng(N + P)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, P))) + 0.1 * rng.standard_normal((N, P))
    gp = GaussianProcessRegressor(kernel=RBF(2.0) + WhiteKernel(0.1), alpha=1e-4, normalize_y=True, optimizer=None,
                                  device=0).fit(X, Y if P > 1 else Y[:, 0])
    dev, ys = gp._dev, gp._y_train_std
    Xq = rng.standard_normal((M, D))
    q = dev._as_queries(Xq, torch.float64)
    dev_ms(lambda: dev.predict_mean_grad_dev(q, ys), 2)
    t_jac = dev_ms(lambda: dev.predict_mean_grad_dev(q, ys), reps)
    dev_ms(lambda: dev.predict_mean_hess_dev(q, ys), 2)
    t_hess = dev_ms(lambda: dev.predict_mean_hess_dev(q, ys), reps)
    # the launch as gpk_predict_mean_hess cuts it at D = 10 (12 padded features): per output two row blocks of the triangle,
    # rows [0, 8) with 36 entries and S, rows [8, 12) with 42 entries; each recomputes the pair's distance and exp
    blocks = ((8, 36 + 1), (4, 42))
    ops = M * N * P * sum(2 * 12 + 20 + 1 + rows + entries for rows, entries in blocks)
    floor_ms = ops / (FP64_VALU_TFLOPS / 2 * 1e12) * 1e3
    a = dev.predict_mean_hess_dev(q[:256], ys).cpu().numpy()
    b = dev.predict_hess_host(Xq[:256], gp._y_train_mean, ys)[2]
    _worst["route"] = max(_worst["route"], relerr(a, b))
    say(f"N = {N:6d} M = {M} P = {P}: predict_mean_grad {t_jac:8.3f} ms  predict_mean_hess {t_hess:8.3f} ms  ratio {t_hess / t_jac:5.2f}  "
        f"vector-issue floor {floor_ms:7.3f} ms ({100 * floor_ms / t_hess:4.1f} % of it reached)")
    del gp, dev
    torch.cuda.empty_cache()


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, N = 16 384 only on the large route")
    ap.add_argument("--log", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    import torch
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        _log = open(a.log, "w")
    say(f"# tools/exp_hess.py on {torch.cuda.get_device_name(0)}; fp64; D = 10")
    reps = 200 if a.quick else 1000
    for N in (1000, 4096):
        single_model(N, reps)
    for N in (1000, 4096):
        axis_models(N, reps)
    sparse_model(1024, reps)
    for N in ((16384,) if a.quick else (16384, 65536)):
        for P in (1, 6):
            large(N, 4096, P, 3 if a.quick else 5)
    for N, B, D in ((4096, 6, 10), (16384, 6, 10)) + (() if a.quick else ((16384, 8, 10), (16384, 6, 16))):
        axis_large(N, 4096, 3 if a.quick else 5, B, D)
    say(f"worst parity: Hessian against the differenced Jacobian calls (h = {FD_H:g}) {_worst['fd']:.1e}; device route against the "
        f"one-call route {_worst['route']:.1e}")


if __name__ == "__main__":
    main()
