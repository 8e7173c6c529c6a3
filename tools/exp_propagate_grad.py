"""Timings of the gradient of a horizon cost through the propagation (K11, `propagate_gradient`: the adjoint chain, one call per
horizon) in one process on one build.

    python tools/exp_propagate_grad.py [--quick] [--log profiles/r26_exp_propagate_grad.log]          (GPK_OPTS=small_path=0,...)

The configurations of tools/exp_propagate2.py (its models and horizons): D = 10, nx = 6, nu = 4, H = 25, R = 1 and 32 rollouts; one
model with P = 6 outputs and six single-output models; exact models at N = 1000 and 4096, sparse models at m = 1024.  Per
configuration, wall time per horizon through the public methods, median of the repetitions after the warm-up calls:

  (a)  `propagate_gradient` as ONE call (6 H launches, one synchronisation) against the host sweep it replaces (`route="host"`: per
       stage `predict_jacobian(return_var=True)` forward and `predict_hessian` backward - 2 H calls, 2 H synchronisations, an
       R x NO x D x D Hessian per stage - with NumPy between them).  The last line says in which configurations, if any, the one
       call is slower.
  (b)  against central differences of `propagate` with respect to the controls: 2 H nu + 1 = 201 calls of the one-call
       `propagate`, the time of one such call (measured here) times 201.
  (c)  against the forward chain alone: `propagate_gradient` / `propagate`, what the backward sweep and the variance gradient's
       third forward launch add.

The two routes of (a) are compared at 1e-10 of the largest component before anything is timed.  The lines are printed and appended
to --log."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exp_propagate2 import D, H, NX, build, horizon, relerr, wall_us  # noqa: E402

ratios = []


def measure(say, tag, model, chain, lin, rng, reps):
    """chain: the route that is the one call ("auto" for the exact classes, "chain" for the sparse ones)"""
    nu = D - NX
    for R in (1, 32):
        x0, U, S0 = horizon(rng, R)
        gx = rng.standard_normal((H + 1, R, NX))
        gS = rng.standard_normal((H + 1, R, NX, NX))
        gS = 0.5 * (gS + gS.transpose(0, 1, 3, 2))
        kw = dict(Sigma0=S0, var_includes_noise=True)
        a = model.propagate_gradient(x0, U, lin, gx, gS, route=chain, **kw)
        b = model.propagate_gradient(x0, U, lin, gx, gS, route="host", **kw)
        agree = max(relerr(x, y) for x, y in zip(a, b))
        assert agree < 1e-10, agree
        tg = wall_us(lambda: model.propagate_gradient(x0, U, lin, gx, gS, route=chain, **kw), reps)
        th = wall_us(lambda: model.propagate_gradient(x0, U, lin, gx, gS, route="host", **kw), min(reps, 40), warm=5)
        t1 = wall_us(lambda: model.propagate(x0, U, lin, route=chain, **kw), reps)
        calls = 2 * H * nu + 1
        ratios.append((f"{tag}, R = {R}", th[0] / tg[0]))
        say(f"{tag}, R = {R:2d}, H = {H}: (a) gradient one call {tg[0]:8.1f} us (p99 {tg[1]:8.1f})   host sweep {th[0]:9.1f} us "
            f"(p99 {th[1]:9.1f})   sweep / one call {th[0] / tg[0]:6.2f}   (b) propagate one call {t1[0]:8.1f} us, x {calls} = "
            f"{calls * t1[0] / 1e3:8.1f} ms, central differences / one call {calls * t1[0] / tg[0]:7.1f}   (c) gradient / propagate "
            f"{tg[0] / t1[0]:5.2f}, {(tg[0] - t1[0]) / H:6.2f} us more per stage   routes agree to {agree:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 1000 only, no sparse models")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "r26_exp_propagate_grad.log"))
    a = ap.parse_args()
    import gpk_opts
    import torch
    gpk_opts.install()      # GPK_OPTS=small_path=0,...: A/B switches
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/exp_propagate_grad.py on {torch.cuda.get_device_name(0)}; fp64; D = {D}, nx = {NX}, H = {H}; wall time per horizon "
        f"through `propagate_gradient` / `propagate`, median of {a.reps} calls after 20 warm-up calls (host sweep: "
        f"{min(a.reps, 40)} after 5); GPK_OPTS = {os.environ.get('GPK_OPTS', '')!r}")
    configs = [("exact one", 1000), ("exact six", 1000)]
    if not a.quick:
        configs += [("exact one", 4096), ("exact six", 4096), ("sparse one", 1024), ("sparse six", 1024)]
    for kind, rows in configs:
        tag, model, chain, lin, rng = build(kind, rows)
        measure(say, tag, model, chain, lin, rng, a.reps)
    slow = [(t, r) for t, r in ratios if r < 1.0]
    say("# (a) the one-call gradient is not slower than the host sweep in any configuration: "
        + ("holds" if not slow else "DOES NOT HOLD: " + ", ".join(f"{t} ({r:.2f})" for t, r in slow)))
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
