"""Measurements of the posterior function draws.

    python tools/exp_paths.py [--quick] [--sizes 1000:1024,4096:2048]

S = 500 paths, P = 6 outputs, D = 10 inputs (the reference's residual model), N = 1000 rows with F = 1024 features and N = 4096
with F = 2048, RBF + WhiteKernel at fixed hyper-parameters.  Per size:

    prepare      gpk_paths_prepare from C (ctypes, device operands in place) up to its synchronisation, and
                 PosteriorPaths.from_randomness from Python (the uploads of W_rand and Eps included)
    step         gpk_paths_step between two device events, queries already on the device: the time of its two launches, and the
                 Coef bytes per second that amounts to, (N + F) S P 8 bytes over that time - a rate of the whole step, the
                 second (combine) launch included, next to the Gram kernel's 5.2 - 5.5 TB/s.  A measurement, not a bar.
    horizon      the 25-stage `rollout` from Python against 25 `step` calls from Python that feed each stage's result back
                 through the host, the two alternated call by call in the same process.  Condition (the only one): the one-call
                 form is not slower.  The last line says whether it holds.
    context      25 `predict` mean calls of 500 rows (no draw: the posterior mean at known points)

Wall-clock figures are the median [min .. max] of samples around calls that end in a synchronisation, after a warm-up.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S, P, D, H = 500, 6, 10, 25


def stats(ts, unit=1e6, name="us"):
    ts = unit * np.asarray(ts)
    return f"{np.median(ts):9.1f} {name} [{ts.min():9.1f} .. {ts.max():9.1f}]"


def timed(fns, reps, warm=5):
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


def model(N):
    from unmanned_aerial_vehicles_amd import RBF, GaussianProcessRegressor, WhiteKernel
    rng = np.random.default_rng(31 * N)
    X = rng.standard_normal((N, D))
    Y = 0.2 * np.sin(X @ rng.standard_normal((D, P))) + 0.05 * rng.standard_normal((N, P))
    gp = GaussianProcessRegressor(RBF(2.0) + WhiteKernel(0.1), alpha=1e-4, normalize_y=True, optimizer=None, device=0).fit(X, Y)
    return gp, rng


def main():
    import torch
    from unmanned_aerial_vehicles_amd import PosteriorPaths, draw_path_randomness
    from unmanned_aerial_vehicles_amd.device import _p
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--sizes", default="1000:1024,4096:2048")
    args = ap.parse_args()
    reps = 10 if args.quick else 40
    verdict = []
    for N, F in [tuple(int(v) for v in x.split(":")) for x in args.sizes.split(",")]:
        gp, rng = model(N)
        tag = f"N = {N:4d} F = {F:4d} S = {S} P = {P}"
        r = draw_path_randomness(np.random.RandomState(0), N, D, F, S, P, 2.0, 0.1 + 1e-4)
        paths = PosteriorPaths.from_randomness(gp, **r)
        be, dev, C = paths.be, paths._dev, S * P
        # ---- prepare
        w_d, e_d = be.upload(r["weights"].reshape(F, C)), be.upload(r["eps"].reshape(N, C))
        coef = be.empty((N + F, C), torch.float64)
        W = dev.inverse_factor(False)

        def prepare_c():
            be.call("gpk_paths_prepare", _p(dev.X), N, D, _p(dev.Yn), P, _p(W), dev.Np, dev.Np, _p(paths._omega), _p(paths._phase), F,
                    paths._sf2, _p(w_d), _p(e_d), S, _p(coef), C)
            be.sync()

        t_c, t_py = timed([prepare_c, lambda: PosteriorPaths.from_randomness(gp, **r)], max(reps // 4, 3), warm=2)
        assert torch.equal(coef, paths.coef)
        print(f"{tag}  prepare from C {stats(t_c, 1e3, 'ms')}   from Python (with uploads) {stats(t_py, 1e3, 'ms')}", flush=True)
        del w_d, e_d, coef
        # ---- step: device events around the C call, queries on the device
        Xs = np.ascontiguousarray(1.2 * rng.standard_normal((S, D)))
        q, out = be.upload(Xs), be.empty((S, P), torch.float64)
        margs = paths._model_args()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10 * reps)]
        for _ in range(20):
            be.call("gpk_paths_step", *margs, _p(q), _p(out))
        for a, b in ev:
            a.record()
            be.call("gpk_paths_step", *margs, _p(q), _p(out))
            b.record()
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        nbytes = (N + F) * C * 8
        print(f"{tag}  step (device events, {len(ev)} calls) {stats(ms, 1e3)}   Coef {nbytes / 1e6:.1f} MB per stage -> "
              f"{nbytes / (np.median(ms) * 1e-3) / 1e12:.2f} TB/s at the median, {nbytes / (ms.min() * 1e-3) / 1e12:.2f} TB/s at the fastest",
              flush=True)
        # ---- the horizon from Python: one rollout call against 25 step calls fed back through the host
        x0 = np.ascontiguousarray(0.3 * rng.standard_normal((S, P)))
        U = np.ascontiguousarray(0.3 * rng.standard_normal((H, D - P)))
        lin = np.zeros((P, D))
        lin[0:3, 3:6] = 0.02 * np.eye(3)
        lin[3:6, 6:9] = 0.02 * np.eye(3)

        def by_steps():
            traj = [x0]
            for u in U:
                x = traj[-1]
                qh = np.concatenate([x, np.broadcast_to(u, (S, D - P))], axis=1)
                traj.append(x + qh @ lin.T + paths.step(qh))
            return np.stack(traj)

        a, b = paths.rollout(x0, U, lin), by_steps()
        err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
        t_roll, t_steps, t_mean = timed([lambda: paths.rollout(x0, U, lin), by_steps, lambda: [gp.predict(Xs) for _ in range(H)]],
                                        reps)
        apart = max(t_roll) < min(t_steps)
        print(f"{tag}  {H}-stage rollout, one call {stats(t_roll, 1e3, 'ms')}   {H} step calls {stats(t_steps, 1e3, 'ms')}   "
              f"steps / rollout {np.median(t_steps) / np.median(t_roll):5.2f} ({'ranges apart' if apart else 'ranges overlap'}; the two agree to "
              f"{err:.1e})   context: {H} predict mean calls of {S} rows {stats(t_mean, 1e3, 'ms')}", flush=True)
        verdict.append((N, F, float(np.median(t_steps) / np.median(t_roll))))
        del paths, gp
    slow = [v for v in verdict if v[2] < 1.0]
    print(f"condition (the one-call rollout is not slower than {H} step calls from Python): "
          f"{'holds' if not slow else 'FAILS for ' + repr(slow)}; steps / rollout " + ", ".join(f"{v[2]:.2f}" for v in verdict))


if __name__ == "__main__":
    main()
