"""Measurements of the path gradients ("path gradients").

    python tools/exp_paths_grad.py [--quick] [--sizes 1000:1024,4096:2048] [--plain-only]

S = 500 paths, D = 10 inputs, at N = 1000 rows with F = 1024 features and N = 4096 with F = 2048: the single model with P = 6
outputs (the problem of tools/exp_paths.py), the per-axis batch with B = 6 (tools/exp_axis_paths.py), and the sparse batch with
B = 6 at m = 1024 inducing inputs, F = 1024 (tools/exp_sparse_paths.py).  Per form, device events around the C calls with the
queries already on the device, the three forms alternated call by call within one run, three rounds:

    plain        the value entry (gpk_paths_step, gpk_paths_step_multi, gpk_paths_step_multi_z)
    grad         the gradient entry on the same arguments (value and Jacobian)
    D + 1 plain  eleven calls of the value entry: the cheapest finite-difference Jacobian a caller had before

Condition: grad beats D + 1 plain at every size; the ratio grad / plain is reported, not prescribed.  The values of the two
entries must agree bit for bit: asserted before anything is timed.  Then the 25-stage rollout from Python, plain against
gradient, wall clock, alternated call by call.  --plain-only times the value entries alone (the same numbers on a build without
the gradient entries: the parent commit's).

Device-event figures are the median of the round medians and the spread of the round medians; [min .. max] over all samples."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exp_sparse_paths import event_rounds, sparse_models, spread, stats, timed  # noqa: E402

S, D, H, NOUT = 500, 10, 25, 6
SPARSE_M, SPARSE_F = 1024, 1024


def forms(N, F):
    """[(tag, path set, value entry, gradient entry)] of one size; the sparse batch only at the first size (its own m and F)"""
    import exp_axis_paths
    import exp_paths
    from unmanned_aerial_vehicles_amd import (BatchedPosteriorPaths, PosteriorPaths, draw_batch_path_randomness, draw_path_randomness)
    gp, _ = exp_paths.model(N)
    r = draw_path_randomness(np.random.RandomState(0), N, D, F, S, NOUT, 2.0, 0.1 + 1e-4)
    yield f"single  N = {N:4d} F = {F:4d} P = {NOUT}", PosteriorPaths.from_randomness(gp, **r), "gpk_paths_step", "gpk_paths_step_grad"
    del gp
    bg, ls, noise, _ = exp_axis_paths.batch(N)
    r = draw_batch_path_randomness(np.random.RandomState(0), N, D, F, S, ls, noise + exp_axis_paths.ALPHA)
    yield (f"batch   N = {N:4d} F = {F:4d} B = {NOUT}", BatchedPosteriorPaths.from_randomness(bg, **r), "gpk_paths_step_multi",
           "gpk_paths_step_multi_grad")


def sparse_form():
    bg, _, _ = sparse_models(SPARSE_M)
    return (f"sparse  m = {SPARSE_M:4d} F = {SPARSE_F:4d} B = {NOUT}", bg.sample_paths(S, n_features=SPARSE_F, random_state=0),
            "gpk_paths_step_multi_z", "gpk_paths_step_multi_grad_z")


def measure(tag, paths, value, grad, n_ev, reps, plain_only, verdict):
    import torch
    from unmanned_aerial_vehicles_amd.device import _p
    be = paths.be
    rng = np.random.default_rng(5)
    q = be.upload(np.ascontiguousarray(1.2 * rng.standard_normal((S, D))))
    out, outg = be.empty((S, NOUT), torch.float64), be.empty((S, NOUT), torch.float64)
    jac = be.empty((S, NOUT, D), torch.float64)
    margs = paths._model_args()

    def plain():
        be.call(value, *margs, _p(q), _p(out))

    def eleven():
        for _ in range(D + 1):
            be.call(value, *margs, _p(q), _p(out))

    if plain_only:
        (rounds,) = event_rounds([plain], n_ev)
        med, spr = spread(rounds)
        print(f"{tag}  plain step {stats(np.concatenate(rounds), 1e3)}   median of the round medians {1e3 * med:8.1f} us, spread "
              f"{100 * spr:4.1f} %", flush=True)
        return

    def gradient():
        be.call(grad, *margs, _p(q), _p(outg), _p(jac))

    plain()
    gradient()
    torch.cuda.synchronize()
    assert torch.equal(out, outg), "the gradient entry's value does not have the bits of the value entry's"
    r_plain, r_grad, r_eleven = event_rounds([plain, gradient, eleven], n_ev)
    (mp, sp), (mg, sg), (me, se) = spread(r_plain), spread(r_grad), spread(r_eleven)
    for name, rounds, med, spr in (("plain step      ", r_plain, mp, sp), ("gradient step   ", r_grad, mg, sg),
                                   (f"{D + 1} plain steps  ", r_eleven, me, se)):
        print(f"{tag}  {name} {stats(np.concatenate(rounds), 1e3)}   median of the round medians {1e3 * med:8.1f} us, spread "
              f"{100 * spr:4.1f} %", flush=True)
    print(f"{tag}  gradient / plain {mg / mp:5.2f}   {D + 1} plain / gradient {me / mg:5.2f}; the values agree bit for bit", flush=True)
    # ---- the 25-stage rollout from Python, plain against gradient
    nx = 6
    x0 = np.ascontiguousarray(0.3 * rng.standard_normal((S, nx)))
    U = np.ascontiguousarray(0.3 * rng.standard_normal((H, D - nx)))
    lin = np.zeros((nx, D))
    lin[0:3, 3:6] = 0.02 * np.eye(3)
    lin[3:6, 6:9] = 0.02 * np.eye(3)
    if hasattr(paths, "set_output_scaler"):
        paths.set_output_scaler(np.zeros(NOUT), np.full(NOUT, 0.05))
    a = paths.rollout(x0, U, lin)
    b, _ = paths.rollout(x0, U, lin, return_jacobian=True)
    assert a.tobytes() == b.tobytes(), "the gradient rollout's trajectory does not have the bits of the plain rollout's"
    t_plain, t_grad = timed([lambda: paths.rollout(x0, U, lin), lambda: paths.rollout(x0, U, lin, return_jacobian=True)], reps)
    print(f"{tag}  {H}-stage rollout {stats(t_plain, 1e3, 'ms')}   with the Jacobians {stats(t_grad, 1e3, 'ms')}   gradient / plain "
          f"{np.median(t_grad) / np.median(t_plain):5.2f}; the trajectories agree bit for bit", flush=True)
    verdict.append((tag, me / mg, mg / mp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--sizes", default="1000:1024,4096:2048")
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    reps = 10 if args.quick else 30
    n_ev = 100 if args.quick else 300
    verdict = []
    for N, F in [tuple(int(v) for v in x.split(":")) for x in args.sizes.split(",")]:
        for tag, paths, value, grad in forms(N, F):
            measure(tag, paths, value, grad, n_ev, reps, args.plain_only, verdict)
            del paths
    measure(*sparse_form(), n_ev, reps, args.plain_only, verdict)
    if not args.plain_only:
        lost = [v[0] for v in verdict if v[1] <= 1.0]
        print(f"condition (a gradient step beats {D + 1} plain steps at every size): {'holds' if not lost else 'FAILS for ' + repr(lost)}; "
              f"{D + 1} plain / gradient " + ", ".join(f"{v[1]:.2f}" for v in verdict) + "; gradient / plain "
              + ", ".join(f"{v[2]:.2f}" for v in verdict))


if __name__ == "__main__":
    main()
