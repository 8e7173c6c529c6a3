"""Timings of the posterior's input gradients (predict_jacobian, K8) against the value calls they extend.

    python tools/exp_jac.py [--quick] [--horizon-only] [--axis]

1. The MPC horizon: 25 rows at N = 1000, D = 10, P = 6: predict_jacobian (mean + Jacobian, one C call) against predict()
   (mean), and predict_jacobian(return_var=True) (all four results) against predict(return_std=True), wall time per call.
2. Large route, N = 16 384 and 65 536, M = 4096 queries, D = 10: the variance-gradient call (gpk_predict_var_grad_inv: K*,
   V = W K*, C = W^T V, one streaming pass) against gpk_predict_var_inv (the fp64 inverse-variance launch); the C = W^T V
   launch alone (event bracket GPK_TIMED_JAC) and its rate on its N^2 M flops; the mean Jacobian (gpk_predict_mean_grad)
   against gpk_predict_mean fp64 on the same queries, with its vector-issue floor; the peak HBM in use during the variance-gradient calls (sampled).
--axis: the per-axis batch (six single-output ARD models on shared inputs, BatchedARDGP) instead of the single model:
3. The MPC horizon: 25 rows of six N = 1000, D = 10 models: the one-call gradient path (gpk_predict_host_multi_grad: ONE launch
   for mean + Jacobian, THREE for all four results - the condition a kernel trace of `--axis --horizon-only` shows) against
   what was there before: gpk_predict_host_multi (mean; mean + std) and six sequential single-model predict_jacobian calls.
4. M = 4096 at N = 4096 and 16 384, B = 6, D = 10: gpk_predict_mean_grad_multi against gpk_predict_mean_multi and against six
   gpk_predict_mean_grad launches, with its share of the fp64 vector-issue floor (counted as in 2.); then the shapes whose
   instantiations run at one wave per SIMD: (B, D) = (8, 10), (6, 16), (8, 16) at N = 16 384.
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


def axis_batch(N, B=6, D=10, seed=0):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, B))) + 0.1 * rng.standard_normal((N, B))
    bg = BatchedARDGP(optimizer=None, device=0)
    for b in range(B):
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.roll(np.linspace(1.2, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))
        bg.models.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=False, optimizer=None, device=0).fit(X, Y[:, b]))
    return bg, rng


def wall_us(fn, reps):
    for _ in range(20):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts)), 1e6 * float(np.percentile(ts, 99))


def axis_horizon(N, M, reps):
    bg, rng = axis_batch(N)
    Xq = np.ascontiguousarray(rng.standard_normal((M, 10)))
    assert bg.predict_host_grad(Xq, True) is not None and bg.predict_host(Xq, True) is not None
    a = wall_us(lambda: bg.predict_host(Xq), reps)
    b = wall_us(lambda: bg.predict_host_grad(Xq), reps)
    c = wall_us(lambda: bg.predict_host(Xq, True), reps)
    e = wall_us(lambda: bg.predict_host_grad(Xq, True), reps)
    f = wall_us(lambda: [m.predict_jacobian(Xq) for m in bg.models], reps)
    g = wall_us(lambda: [m.predict_jacobian(Xq, return_var=True) for m in bg.models], reps)
    print(f"per-axis B = 6, N = {N} rows = {M}: host_multi mean {a[0]:7.1f} us (p99 {a[1]:7.1f})   one-call mean+Jacobian "
          f"{b[0]:7.1f} us (p99 {b[1]:7.1f})   ratio {b[0] / a[0]:5.3f}   six predict_jacobian calls {f[0]:7.1f} us "
          f"(p99 {f[1]:7.1f}): {f[0] / b[0]:5.2f} x the one call", flush=True)
    print(f"per-axis B = 6, N = {N} rows = {M}: host_multi mean+std {c[0]:7.1f} us (p99 {c[1]:7.1f})   one-call all four results "
          f"{e[0]:7.1f} us (p99 {e[1]:7.1f})   ratio {e[0] / c[0]:5.3f}   six predict_jacobian(return_var) calls {g[0]:7.1f} us "
          f"(p99 {g[1]:7.1f}): {g[0] / e[0]:5.2f} x the one call", flush=True)


def axis_large(N, M, reps, B=6, D=10):
    import ctypes as C
    import torch
    from unmanned_aerial_vehicles_amd import _lib
    from unmanned_aerial_vehicles_amd.device import get_backend
    bg, rng = axis_batch(N, B, D)
    f = bg._fused64()
    be = get_backend(0)
    q = be.upload(np.ascontiguousarray(rng.standard_normal((M, D))), torch.float64)
    mean, dmean = be.empty((M, B), torch.float64), be.empty((M, B, D), torch.float64)
    dp = _lib._dp
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ls, sf2, ym, ys = (f[k].ctypes.data_as(dp) for k in ("ls", "sf2", "ym", "ys"))

    def fused_mean():
        with be.lock:
            be.bind_stream()
            be.check(be.lib.gpk_predict_mean_multi(be.h, _lib.GPK_F64, p(f["X"]), p(f["alpha"]), N, D, B, ls, sf2, ym, ys, p(q), M, p(mean)))

    def fused_jac():
        with be.lock:
            be.bind_stream()
            be.check(be.lib.gpk_predict_mean_grad_multi(be.h, p(f["X"]), p(f["alpha"]), N, D, B, ls, sf2, ys, p(q), M, p(dmean)))

    def six_jac():
        for m in bg.models:
            m._dev.predict_mean_grad_dev(q, m._y_train_std)

    for fn in (fused_mean, fused_jac, six_jac):
        dev_ms(fn, 2)
    t_mean, t_jac, t_six = dev_ms(fused_mean, reps), dev_ms(fused_jac, reps), dev_ms(six_jac, reps)
    # vector-issue floor, counted as for the single model: per pair D subtracts once, then per model D multiplies + D FMAs
    # (distance) + ~20 (exp) + 1 (weight) + D FMAs (sums)
    ops = M * N * (D + B * (2 * D + 20 + 1 + D))
    floor_ms = ops / (FP64_VALU_TFLOPS / 2 * 1e12) * 1e3
    print(f"per-axis B = {B}, D = {D}, N = {N:6d} M = {M}: predict_mean_multi {t_mean:8.3f} ms  predict_mean_grad_multi {t_jac:8.3f} ms  "
          f"ratio {t_jac / t_mean:5.2f}  {B} predict_mean_grad launches {t_six:8.3f} ms ({t_six / t_jac:5.2f} x)  "
          f"vector-issue floor {floor_ms:6.3f} ms ({100 * floor_ms / t_jac:4.1f} % of it reached)", flush=True)
    del bg
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 16 384 only, fewer repetitions")
    ap.add_argument("--horizon-only", action="store_true", help="the control-loop timings only (for a kernel trace)")
    ap.add_argument("--axis", action="store_true", help="the per-axis batch (six single-output models) instead of the single model")
    a = ap.parse_args()
    import torch
    print(f"# tools/exp_jac.py on {torch.cuda.get_device_name(0)}; fp64; D = 10", flush=True)
    if a.axis:
        axis_horizon(1000, 25, 200 if a.quick or a.horizon_only else 1000)
        if not a.horizon_only:
            for N in (4096, 16384):
                axis_large(N, 4096, 3 if a.quick else 5)
            # the instantiations that run at one wave per SIMD (256 VGPRs + accumulation registers): <3,4>, <4,3>, <4,4>
            for B, D in ((8, 10), (6, 16), (8, 16)):
                axis_large(16384, 4096, 3 if a.quick else 5, B, D)
        return
    horizon(1000, 25, 200 if a.quick or a.horizon_only else 1000)
    if a.horizon_only:
        return
    for N in ((16384,) if a.quick else (16384, 65536)):
        large(N, 4096, 3 if a.quick else 5)


if __name__ == "__main__":
    main()
