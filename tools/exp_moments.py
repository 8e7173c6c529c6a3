"""Exact moment matching (K11, method="moment"): what it costs on the GPU and what it buys, in one log.

    python tools/exp_moments.py [--quick] [--table-only] [--log profiles/r27_exp_moments.log]

Timings (GPU).  D = 10, nx = 6, H = 25, R = 1 and 32 rollouts; one model with P = 6 outputs at N = 1000 and 4096, and six
per-axis models (BatchedARDGP) at the same N - the problems of tools/exp_propagate.py.  Per configuration, wall time per horizon,
median of the repetitions after warm-up:

  mm     `propagate(method="moment")`: the one-call chain (5 H launches, one synchronisation);
  host   `propagate(method="moment", route="host")`: H `predict_moments` calls (5 launches and one synchronisation each) around
         the composition on the host;
  lin    `propagate()`: the first-order chain (3 H launches, one synchronisation);
  fin    the finishing launch of a stage alone (event bracket GPK_TIMED_PROPAGATE), and from the H brackets of one call the
         number of synchronisations: the brackets of one horizon are all read back after the call's ONE synchronisation.

Accuracy (CPU, NumPy forms of tests/).  On the four models of tests/golden/paths_ref.npz at Sigma = 6.25e-3 V V^T, one stage:
error of the mean x_1 and of Sigma_1 of the linear recursion, of order=2 and of the exact moments against tensor Gauss-Hermite
quadrature of the model's own posterior (12 nodes per dimension; csv, nx = 6: 6 nodes), relative to the largest entry.

The lines are printed and appended to --log."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def accuracy_table(say):
    from test_moments_host import CASES, form_of, gauss_hermite, gaussian_query, rel
    from test_propagate2_host import second
    say("# one stage at Sigma = 6.25e-3 V V^T against Gauss-Hermite quadrature: relative error of x_1 / of Sigma_1")
    for name in sorted(CASES):
        c, pform, mform = form_of(name)
        lin = c["lin"]
        nx = lin.shape[0]
        q, S = gaussian_query(c, 6.25e-3)
        m, V, xc = gauss_hermite(pform, q, S, CASES[name])
        A0 = np.eye(nx) + lin[:, :nx]
        F = A0 @ xc[:, :nx].T
        x1 = q[:nx] + lin @ q + m
        S1 = A0 @ S @ A0.T + F + F.T + V
        x0, U = q[None, :nx], q[None, None, nx:]
        rows = []
        lt, lS, _ = pform.run(x0, U, lin, S[None])
        st, sS, _ = second(pform).run2(x0, U, lin, S[None])
        mt, mS, _ = mform.run(range(nx), x0, U, lin, S[None])
        for tag, t, s in (("linear", lt, lS), ("order=2", st, sS), ("moment", mt, mS)):
            rows.append(f"{tag} {rel(t[1, 0], x1):.1e} / {rel(s[1, 0], S1):.1e}")
        say(f"case {name:3s} (N = {len(c['X'])}, nx = {nx}): " + "   ".join(rows))


def timings(say, N, reps):
    from exp_propagate import H, NX, horizon, problem, relerr, wall_us
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel, _lib
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    D = 10
    X, Y, lin, rng = problem(N)
    gp = GaussianProcessRegressor(kernel=RBF(2.0) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X, Y)
    X2, Y2, _, rng2 = problem(N, 1)
    bg = BatchedARDGP(optimizer=None, device=0)
    for b in range(NX):
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.roll(np.linspace(1.5, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))
        bg.models.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X2, Y2[:, b]))
    S0 = 1e-3 * np.eye(NX)
    for tag, model, dev in (("one model P = 6", gp, gp._dev), ("six per-axis models", bg, bg.models[0]._dev)):
        for R in (1, 32):
            x0, U = horizon(rng, R)
            mm = lambda: model.propagate(x0, U, lin, Sigma0=S0, method="moment")                    # noqa: E731
            host = lambda: model.propagate(x0, U, lin, Sigma0=S0, method="moment", route="host")   # noqa: E731
            first = lambda: model.propagate(x0, U, lin, Sigma0=S0)                                   # noqa: E731
            a, b = mm(), host()
            agree = max(relerr(a[0], b[0]), relerr(a[1], b[1]))
            assert agree < 1e-8, agree
            r_mm = max(3, reps // (8 if R == 32 else 1))
            t_mm, t_lin = wall_us(mm, r_mm, warm=2), wall_us(first, reps)
            t_host = wall_us(host, max(2, r_mm // 3), warm=1)
            dev.timing(True)
            mm()
            fin = dev.kernel_times(_lib.GPK_TIMED_PROPAGATE)
            dev.timing(False)
            say(f"{tag}, N = {N:5d}, R = {R:2d}, H = {H}: mm {t_mm[0]:10.1f} us   host {t_host[0]:10.1f} us   lin {t_lin[0]:8.1f} us   "
                f"mm / lin {t_mm[0] / t_lin[0]:7.1f}   host / mm {t_host[0] / t_mm[0]:5.2f}   fin {1e3 * float(np.median(fin)):5.1f} us, "
                f"{len(fin)} brackets read after the call's one synchronisation   routes agree to {agree:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 1000 only")
    ap.add_argument("--table-only", action="store_true", help="the CPU accuracy table alone (no GPU)")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r27_exp_moments.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not a.table_only:
        import torch
        say(f"# tools/exp_moments.py on {torch.cuda.get_device_name(0)}; fp64; D = 10, nx = 6, H = 25, Sigma0 = 1e-3 I; wall time per "
            f"horizon, median of up to {a.reps} calls after warm-up")
        for N in ((1000,) if a.quick else (1000, 4096)):
            timings(say, N, a.reps)
    accuracy_table(say)
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
