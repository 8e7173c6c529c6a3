"""The gradient through exact moment matching (`propagate_moments_gradient`): what it costs on the GPU, in one log.

    python tools/exp_moments_grad.py [--quick] [--forward-only] [--log profiles/r29_exp_moments_grad.log]

D = 10, nx = 6, H = 25, R = 1 and 32 rollouts; one model with P = 6 outputs at N = 1000 and 4096, and six per-axis models
(BatchedARDGP) at the same N - the problems of tools/exp_moments.py.  Per configuration, wall time per horizon, the median over
alternating rounds (one call of every arm per round, after warm-up):

  grad   `propagate_moments_gradient`: the one-call chain (6 H launches forward, 7 H backward, one synchronisation);
  fwd    `propagate(method="moment")`: the forward chain (5 H launches), whose kernels this feature left as they were;
         --forward-only times this arm alone (another build of the library through GPK_LIBRARY);
  fd     what central differences over the forward call cost: fwd x 2 (H nu + nx);
  host   `propagate_moments_gradient(route="host")`: one forward chain and H `predict_moments_vjp` calls.

From grad - fwd at R = 32 the log also gives the pairs of training rows per second that the backward sweep gets through (its row
recomputation and small launches included: a lower bound for the pair launch).  The lines are printed and appended to --log."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rounds(arms, n, warm=1):
    """median wall time (us) of every arm over n alternating rounds"""
    for _ in range(warm):
        for f in arms:
            f()
    t = np.zeros((n, len(arms)))
    for i in range(n):
        for j, f in enumerate(arms):
            t0 = time.perf_counter()
            f()
            t[i, j] = 1e6 * (time.perf_counter() - t0)
    return np.median(t, axis=0), np.min(t, axis=0)


def timings(say, N, reps, forward_only):
    from exp_propagate import H, NX, horizon, problem, relerr
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    D = 10
    nu = D - NX
    X, Y, lin, rng = problem(N)
    gp = GaussianProcessRegressor(kernel=RBF(2.0) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X, Y)
    X2, Y2, _, rng2 = problem(N, 1)
    bg = BatchedARDGP(optimizer=None, device=0)
    for b in range(NX):
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.roll(np.linspace(1.5, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))
        bg.models.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X2, Y2[:, b]))
    S0 = 1e-3 * np.eye(NX)
    seeds = np.random.default_rng(29)
    for tag, model, pairs in (("one model P = 6", gp, 1), ("six per-axis models", bg, NX * (NX + 1) // 2)):
        for R in (1, 32):
            x0, U = horizon(rng, R)
            gx, gS = seeds.standard_normal((H + 1, R, NX)), seeds.standard_normal((H + 1, R, NX, NX))
            fwd = lambda: model.propagate(x0, U, lin, Sigma0=S0, method="moment")      # noqa: E731
            n = max(3, reps // (8 if R == 32 else 1) // (4 if N > 2000 else 1))
            if forward_only:
                (t_fwd,), (m_fwd,) = rounds([fwd], n)
                say(f"{tag}, N = {N:5d}, R = {R:2d}, H = {H}: fwd {t_fwd:10.1f} us (min {m_fwd:10.1f})   [{n} rounds]")
                continue
            grad = lambda: model.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0)                   # noqa: E731
            host = lambda: model.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, route="host")     # noqa: E731
            a, b = grad(), host()
            agree = max(relerr(a[k], b[k]) for k in (2, 3, 4))
            assert agree < 1e-8, agree
            (t_grad, t_fwd, t_host), (m_grad, m_fwd, m_host) = rounds([grad, fwd, host], n)
            back = (t_grad - t_fwd) * 1e-6
            rate = pairs * float(N) * N * R * H / back if R == 32 else 0.0
            say(f"{tag}, N = {N:5d}, R = {R:2d}, H = {H}: grad {t_grad:10.1f} us (min {m_grad:10.1f})   fwd {t_fwd:10.1f} us (min "
                f"{m_fwd:10.1f})   grad / fwd {t_grad / t_fwd:5.2f}   fd = fwd x {2 * (H * nu + NX)}: {t_fwd * 2 * (H * nu + NX) * 1e-3:9.1f} ms, "
                f"fd / grad {t_fwd * 2 * (H * nu + NX) / t_grad:6.1f}   host {t_host:10.1f} us, host / grad {t_host / t_grad:5.2f}"
                + (f"   backward sweep {rate:.3e} pairs of rows / s" if rate else "") + f"   routes agree to {agree:.1e}   [{n} rounds]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 1000 only")
    ap.add_argument("--forward-only", action="store_true", help="the forward arm alone (a run of another build through GPK_LIBRARY)")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r29_exp_moments_grad.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    lib = os.environ.get("GPK_LIBRARY")
    say(f"# tools/exp_moments_grad.py on {torch.cuda.get_device_name(0)}; fp64; D = 10, nx = 6, H = 25, Sigma0 = 1e-3 I; wall time per "
        f"horizon, median over alternating rounds" + (f"; library {os.path.basename(os.path.dirname(lib))}/{os.path.basename(lib)}" if lib else ""))
    for N in ((1000,) if a.quick else (1000, 4096)):
        timings(say, N, a.reps, a.forward_only)
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
