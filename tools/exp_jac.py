"""Timings of the posterior's input gradients (predict_jacobian, K8) against the value calls they extend.

    python tools/exp_jac.py [--quick]

1. The MPC horizon: 25 rows at N = 1000, D = 10, P = 6: predict_jacobian (mean + Jacobian, one C call) against predict()
   (mean), and predict_jacobian(return_var=True) (all four results) against predict(return_std=True), wall time per call.
2. Large route, N = 16 384 and 65 536, M = 4096 queries, D = 10: the variance-gradient call (gpk_predict_var_grad_inv: K*,
   V = W K*, C = W^T V, one streaming pass) against gpk_predict_var_inv (the fp64 inverse-variance launch); the C = W^T V
   launch alone (event bracket GPK_TIMED_JAC) and its rate on its N^2 M flops; the mean Jacobian (gpk_predict_mean_grad)
   against gpk_predict_mean fp64 on the same queries, with its vector-issue floor; the peak HBM in use during the variance-gradient calls (sampled).
Medians over the repetitions; CUDA events around the device calls, perf_counter around the estimator calls."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VALU_TFLOPS = 78.6      # MI355X fp64 vector peak (FMA = 2 flops), the same figure as the fp64 matrix peak


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


class PeakHBM:
    """Peak device memory in use while the block runs, whoever allocated it (torch's caching allocator, the library's own
    hipMalloc'd scratch and staging): a host thread samples hipMemGetInfo every millisecond; `gib` = total - lowest free."""

    def __enter__(self):
        import threading
        import torch
        self._torch = torch
        free, self.total = torch.cuda.mem_get_info(0)
        self.min_free = free
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def _run(self):
        while not self._stop.is_set():
            self.min_free = min(self.min_free, self._torch.cuda.mem_get_info(0)[0])
            time.sleep(1e-3)

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.min_free = min(self.min_free, self._torch.cuda.mem_get_info(0)[0])
        self.gib = (self.total - self.min_free) / 2 ** 30


def large(N, M, reps):
    import torch
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel, _lib
    rng = np.random.default_rng(N)
    D, P = 10, 1
    X = rng.standard_normal((N, D))
    y = np.sin(X @ rng.standard_normal(D)) + 0.1 * rng.standard_normal(N)
    gp = GaussianProcessRegressor(kernel=RBF(2.0) + WhiteKernel(0.1), alpha=1e-4, normalize_y=True, optimizer=None,
                                  device=0).fit(X, y)
    dev = gp._dev
    dev.inverse_factor(False)
    q = dev._as_queries(rng.standard_normal((M, D)), torch.float64)
    kss = 1.1
    ys = gp._y_train_std
    dev_ms(lambda: dev.predict_var_dev(q, kss, 0.0, "float64", "inverse"), 2)
    t_var = dev_ms(lambda: dev.predict_var_dev(q, kss, 0.0, "float64", "inverse"), reps)
    dev_ms(lambda: dev.predict_mean_dev(q, gp._y_train_mean, ys, "float64"), 2)
    t_mean = dev_ms(lambda: dev.predict_mean_dev(q, gp._y_train_mean, ys, "float64"), reps)
    dev_ms(lambda: dev.predict_mean_grad_dev(q, ys), 2)
    t_jac = dev_ms(lambda: dev.predict_mean_grad_dev(q, ys), reps)
    # the variance-gradient call itself (like predict_var_dev it allocates its work panels inside the bracket), with the
    # free HBM sampled from a host thread while it runs: the lowest reading gives the peak in use
    dev_ms(lambda: dev.predict_var_grad_dev(q, kss, 0.0), 2)
    with PeakHBM() as peak:
        t_vg = dev_ms(lambda: dev.predict_var_grad_dev(q, kss, 0.0), reps)
    dev.timing(True)
    for _ in range(reps):
        dev.predict_var_grad_dev(q, kss, 0.0)
    t_wtv = float(np.median(dev.kernel_times(_lib.GPK_TIMED_JAC)))
    dev.timing(False)
    Np, Mp = dev.Np, (M + 127) // 128 * 128
    # FLOPS (one multiply-add = 2 flops) of the launch: the lower 128 x 128 tiles of W incl. the diagonal ones hold
    # Np (Np + 128) / 2 entries, each in Mp multiply-adds: 2 * Np (Np + 128) / 2 * Mp = N^2 M (1 + 128 / N) flops, set against
    # the 78.6 TFLOP/s fp64 matrix peak (the accounting of var_inv's N^2 M flops and of tools/exp_cov.py's N M^2)
    tf = Np * (Np + 128) * Mp / (t_wtv * 1e-3) / 1e12
    # vector-issue floor of the mean Jacobian: per pair D subtract + D FMA (distance) + ~20 (exp) + P (weights) + D P FMAs,
    # every fp64 vector instruction at the FMA rate
    ops = M * N * (2 * D + 20 + P + D * P)
    floor_ms = ops / (FP64_VALU_TFLOPS / 2 * 1e12) * 1e3
    print(f"N = {N:6d} M = {M}: var_inv {t_var:8.2f} ms  var_grad_inv {t_vg:8.2f} ms  ratio {t_vg / t_var:5.3f}  "
          f"W^T V launch {t_wtv:7.2f} ms = {tf:5.1f} TFLOP/s on its N^2 M flops ({100 * tf / 78.6:4.1f} % of 78.6)", flush=True)
    print(f"N = {N:6d} M = {M}: predict_mean {t_mean:8.3f} ms  predict_mean_grad {t_jac:8.3f} ms  ratio {t_jac / t_mean:5.2f}  "
          f"vector-issue floor {floor_ms:6.3f} ms ({100 * floor_ms / t_jac:4.1f} % of it reached)   "
          f"peak HBM in use during the variance-gradient calls {peak.gib:6.1f} GiB", flush=True)
    del gp, dev
    torch.cuda.empty_cache()


def horizon(N, M, reps):
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    d = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "csv_170501.npz"))
    X, Y = d["X10"][:N], d["Y6"][:N]
    gp = GaussianProcessRegressor(kernel=RBF(0.5) + WhiteKernel(0.1), alpha=1e-4, normalize_y=True, optimizer=None,
                                  device=0).fit(X, Y)
    Xq = np.ascontiguousarray(d["Xq10"][:M])

    def wall(fn):
        for _ in range(20):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return 1e6 * float(np.median(ts)), 1e6 * float(np.percentile(ts, 99))

    a = wall(lambda: gp.predict(Xq))
    b = wall(lambda: gp.predict_jacobian(Xq))
    c = wall(lambda: gp.predict(Xq, return_std=True))
    e = wall(lambda: gp.predict_jacobian(Xq, return_var=True))
    print(f"N = {N} rows = {M}: predict() mean {a[0]:7.1f} us (p99 {a[1]:7.1f})   mean+Jacobian {b[0]:7.1f} us "
          f"(p99 {b[1]:7.1f})   ratio {b[0] / a[0]:5.3f}", flush=True)
    print(f"N = {N} rows = {M}: predict() mean+std {c[0]:7.1f} us (p99 {c[1]:7.1f})   all four results {e[0]:7.1f} us "
          f"(p99 {e[1]:7.1f})   ratio {e[0] / c[0]:5.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 16 384 only, fewer repetitions")
    ap.add_argument("--horizon-only", action="store_true", help="the control-loop timings only (for a kernel trace)")
    a = ap.parse_args()
    import torch
    print(f"# tools/exp_jac.py on {torch.cuda.get_device_name(0)}; fp64; D = 10", flush=True)
    horizon(1000, 25, 200 if a.quick or a.horizon_only else 1000)
    if a.horizon_only:
        return
    for N in ((16384,) if a.quick else (16384, 65536)):
        large(N, 4096, 3 if a.quick else 5)


if __name__ == "__main__":
    main()
