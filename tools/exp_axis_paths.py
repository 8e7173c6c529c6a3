"""Measurements of the posterior function draws of the per-axis batch ("the per-axis batch").

    python tools/exp_axis_paths.py [--quick] [--sizes 1000:1024,4096:2048]

B = 6 single-output models on shared inputs, each with its own length-scales and noise (the trained model file's shape),
S = 500 paths, D = 10 inputs, N = 1000 rows with F = 1024 features and N = 4096 with F = 2048.  Per size:

    step         gpk_paths_step_multi between two device events, queries already on the device: the time of its two launches,
                 and the Coef bytes per second that amounts to, (N + F) S B 8 bytes over that time.  In the same run, alternated
                 sample by sample: the six gpk_paths_step calls (P = 1, one per model on its own path set of the same randomness;
                 twelve launches, the same bytes) that the one call replaces, between two device events as well.  Column b of
                 the batch's result must have the bits of model b's own call: asserted before anything is timed.
                 Expectation, not a promise: the batch step is not slower than the six calls.  The numbers are printed either
                 way.
    horizon      the 25-stage `rollout` from Python against 25 `step` calls from Python that feed each stage's result back
                 through the host, alternated call by call in the same process.  Condition: the one-call form is not slower.

Device-event figures are the median [min .. max] over at least 200 calls after a warm-up; wall-clock figures the same over
samples around calls that end in a synchronisation.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S, B, D, H = 500, 6, 10, 25
ALPHA = 1e-4


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


def batch(N):
    from unmanned_aerial_vehicles_amd import RBF, BatchedARDGP, GaussianProcessRegressor, WhiteKernel
    rng = np.random.default_rng(37 * N)
    X = rng.standard_normal((N, D))
    Y = 0.2 * np.sin(X @ rng.standard_normal((D, B))) + 0.05 * rng.standard_normal((N, B))
    ls = np.stack([2.0 * (1.0 + 0.05 * np.arange(D)) * (1.0 + 0.1 * b) for b in range(B)])
    noise = 0.1 * (1.0 + 0.2 * np.arange(B))
    bg = BatchedARDGP(optimizer=None, alpha=ALPHA, normalize_y=True, device=0)
    bg.models = [GaussianProcessRegressor(RBF(ls[b]) + WhiteKernel(noise[b]), alpha=ALPHA, normalize_y=True, optimizer=None,
                                          device=0).fit(X, Y[:, b]) for b in range(B)]
    return bg, ls, noise, rng


def main():
    import torch
    from unmanned_aerial_vehicles_amd import BatchedPosteriorPaths, PosteriorPaths, draw_batch_path_randomness
    from unmanned_aerial_vehicles_amd.device import _p
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--sizes", default="1000:1024,4096:2048")
    args = ap.parse_args()
    reps = 10 if args.quick else 40
    n_ev = 200 if args.quick else 400
    verdict = []
    for N, F in [tuple(int(v) for v in x.split(":")) for x in args.sizes.split(",")]:
        bg, ls, noise, rng = batch(N)
        tag = f"N = {N:4d} F = {F:4d} S = {S} B = {B}"
        r = draw_batch_path_randomness(np.random.RandomState(0), N, D, F, S, ls, noise + ALPHA)
        t0 = time.perf_counter()
        paths = BatchedPosteriorPaths.from_randomness(bg, **r)
        t_prep = time.perf_counter() - t0
        singles = [PosteriorPaths.from_randomness(bg.models[b], r["omega"][b], r["phase"][b], r["weights"][b], r["eps"][b])
                   for b in range(B)]
        be = paths.be
        # ---- step: device events around the C calls, queries on the device
        Xs = np.ascontiguousarray(1.2 * rng.standard_normal((S, D)))
        q, out = be.upload(Xs), be.empty((S, B), torch.float64)
        outs = [be.empty((S, 1), torch.float64) for _ in range(B)]
        margs, sargs = paths._model_args(), [p._model_args() for p in singles]

        def one_call():
            be.call("gpk_paths_step_multi", *margs, _p(q), _p(out))

        def six_calls():
            for b in range(B):
                singles[b].be.call("gpk_paths_step", *sargs[b], _p(q), _p(outs[b]))

        one_call()
        six_calls()
        torch.cuda.synchronize()
        same = all(torch.equal(out[:, b], outs[b][:, 0]) for b in range(B))
        assert same, "a column of the batch step does not have the bits of its model's own step"
        evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_ev)] for _ in range(2)]
        for _ in range(20):
            one_call()
            six_calls()
        for k in range(n_ev):
            for fn, ev in ((one_call, evs[0][k]), (six_calls, evs[1][k])):
                ev[0].record()
                fn()
                ev[1].record()
        torch.cuda.synchronize()
        ms1, ms6 = (np.array([a.elapsed_time(b) for a, b in ev]) for ev in evs)
        nbytes = (N + F) * S * B * 8
        print(f"{tag}  set-up from Python (six gpk_paths_prepare, uploads included) {1e3 * t_prep:.1f} ms", flush=True)
        print(f"{tag}  batch step (device events, {n_ev} calls) {stats(ms1, 1e3)}   Coef {nbytes / 1e6:.1f} MB per stage -> "
              f"{nbytes / (np.median(ms1) * 1e-3) / 1e12:.2f} TB/s at the median, {nbytes / (ms1.min() * 1e-3) / 1e12:.2f} TB/s at the "
              f"fastest", flush=True)
        print(f"{tag}  six gpk_paths_step calls, P = 1 (device events, {n_ev} samples) {stats(ms6, 1e3)}   -> "
              f"{nbytes / (np.median(ms6) * 1e-3) / 1e12:.2f} TB/s at the median   six / batch {np.median(ms6) / np.median(ms1):5.2f}; "
              f"the columns agree bit for bit", flush=True)
        # ---- the horizon from Python: one rollout call against 25 step calls fed back through the host
        nx = 6
        x0 = np.ascontiguousarray(0.3 * rng.standard_normal((S, nx)))
        U = np.ascontiguousarray(0.3 * rng.standard_normal((H, D - nx)))
        lin = np.zeros((nx, D))
        lin[0:3, 3:6] = 0.02 * np.eye(3)
        lin[3:6, 6:9] = 0.02 * np.eye(3)
        sc = (0.1 * rng.standard_normal(D), 1.0 + 0.2 * rng.random(D))
        paths.set_output_scaler(np.zeros(B), np.full(B, 0.05))

        def by_steps():
            traj = [x0]
            for u in U:
                x = traj[-1]
                qh = np.concatenate([x, np.broadcast_to(u, (S, D - nx))], axis=1)
                traj.append(x + qh @ lin.T + paths.step((qh - sc[0]) / sc[1]))
            return np.stack(traj)

        def by_rollout():
            return paths.rollout(x0, U, lin, in_scaler=sc)

        a, b = by_rollout(), by_steps()
        err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
        t_roll, t_steps = timed([by_rollout, by_steps], reps)
        apart = max(t_roll) < min(t_steps)
        print(f"{tag}  {H}-stage rollout, one call {stats(t_roll, 1e3, 'ms')}   {H} step calls {stats(t_steps, 1e3, 'ms')}   "
              f"steps / rollout {np.median(t_steps) / np.median(t_roll):5.2f} ({'ranges apart' if apart else 'ranges overlap'}; the two agree to "
              f"{err:.1e})", flush=True)
        verdict.append((N, F, float(np.median(ms6) / np.median(ms1)), float(np.median(t_steps) / np.median(t_roll))))
        del paths, singles, bg
    slow = [v[:2] for v in verdict if v[3] < 1.0]
    print(f"condition (the one-call rollout is not slower than {H} step calls from Python): "
          f"{'holds' if not slow else 'FAILS for ' + repr(slow)}; steps / rollout " + ", ".join(f"{v[3]:.2f}" for v in verdict))
    behind = [v[:2] for v in verdict if v[2] < 1.0]
    print("expectation (the batch step is not slower than the six calls it replaces): "
          f"{'met' if not behind else 'NOT met for ' + repr(behind)}; six / batch " + ", ".join(f"{v[2]:.2f}" for v in verdict))


if __name__ == "__main__":
    main()
