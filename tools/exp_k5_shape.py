#!/usr/bin/env python3
"""The two MFMA shapes of the fp16 x 2 variance launch (handle option k5_mfma_shape: 1 = 32x32x16, 2 = 16x16x32) against each other
inside ONE process, on one fitted model at the headline shape (N = 65 536, 10 000 queries):

    python tools/exp_k5_shape.py [--n 65536] [--m 10000] [--reps 12] [--warm-s 2.0] [--arms 1,2,1,2] [--log FILE]

Per arm: back-to-back launches of gpk_predict_var_inv_split2 for at least --warm-s seconds, then --reps launches whose kernel times
come from the library's own event ring (GPK_TIMED_K5); mean / min / max, the rate, the error of the standard deviation against the
fp64 kernels, and the largest difference to the first arm's variances.  The whole-benchmark comparison (bench.py under
the parent commit's build, this build and the parent's again, each through GPK_LIBRARY) is a job of its own; its lines are kept
next to this log."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from unmanned_aerial_vehicles_amd import _lib  # noqa: E402
from unmanned_aerial_vehicles_amd.device import DeviceGP, get_backend  # noqa: E402

NAME = {1: "32x32x16", 2: "16x16x32"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warm-s", type=float, default=2.0)
    ap.add_argument("--arms", default="1,2,1,2")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    out = open(args.log, "w") if args.log else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    be = get_backend(0)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((args.n, 9))
    Y = np.sin(X @ rng.standard_normal((9, 3))) + 0.1 * rng.standard_normal((args.n, 3))
    dev = DeviceGP(X, (Y - Y.mean(0)) / Y.std(0), be)
    dev.factorize(2.0, 1.0, 0.1 + 1e-4)
    q = torch.as_tensor(np.random.default_rng(1).standard_normal((args.m, 9)), dtype=torch.float32, device=be.device)
    v64 = dev.predict_var_dev(q.double(), 1.1, 0.0, "float64", "inverse")
    dev.inverse_factor(True)
    dev._Winv.pop("f64", None)
    dev.split2_inverse_factor()
    dev._Winv.pop("f32", None)
    say(f"== tools/exp_k5_shape.py: N {args.n}, {args.m} queries, arms {args.arms}, {args.reps} timed launches per arm after >= {args.warm_s} s of warm launches")
    first = None
    for arm in (int(a) for a in args.arms.split(",")):
        be.check(be.lib.gpk_set_option(be.h, b"k5_mfma_shape", arm))
        t0, warm = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.warm_s:
            dev.predict_var_dev(q, 1.1, 0.0, "float32", "inverse_split2")
            torch.cuda.synchronize()
            warm += 1
        dev.timing(True)
        for _ in range(args.reps):
            v = dev.predict_var_dev(q, 1.1, 0.0, "float32", "inverse_split2")
        ms = dev.kernel_times(_lib.GPK_TIMED_K5)
        dev.timing(False)
        err = float(((v.sqrt() - v64.sqrt()).abs() / v64.sqrt()).max())
        first = v.clone() if first is None else first
        say(f"shape {arm} ({NAME[arm]}): {warm:3d} warm, kernel {np.mean(ms):8.3f} ms (min {np.min(ms):.3f} max {np.max(ms):.3f}, n {len(ms)}) = "
            f"{3.0 * args.n * args.n * args.m / np.mean(ms) / 1e9:7.1f} TF issued, {args.m / np.mean(ms):6.1f} k pred/s kernel-only; "
            f"std err vs fp64 {err:.2e}; max |v - v(first arm)| / v {float(((v - first).abs() / first).max()):.2e}")
    be.check(be.lib.gpk_set_option(be.h, b"k5_mfma_shape", 0))


if __name__ == "__main__":
    main()
