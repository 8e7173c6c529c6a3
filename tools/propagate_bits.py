#!/usr/bin/env python3
"""SHA-256 of everything the horizon-propagation family returns, through the package: one line per result.  Two
trees - library and Python layer - compute the same bits exactly when the two outputs are equal:
    python tools/propagate_bits.py > new.txt;  (cd /path/to/other/tree && python tools/propagate_bits.py) > old.txt
    python tools/propagate_bits.py --compare old.txt new.txt
    python tools/propagate_bits.py --condense new.txt          (one line per model and chain: the record kept under profiles/)
The models and horizons are the tests' own (their `case` / `problem` / `served` functions): every case of
tests/test_gpu_propagate.py, _propagate2, _propagate_grad and _moments on the exact single model, of _axis_propagate on the exact
batch, of _sparse_propagate and _sparse_propagate2 on the sparse classes (route="chain"), each at R = 1 and 5, with Sigma0 = 0 and
with an SPD Sigma0 and Q, with the noise level and without: traj, Sigma and every stage array at orders 1 and 2 (corr with it),
the gradient chain's dU, dx0, dSigma0 with the seed gS and without, the moment chain's stages, `predict_moments`' three results,
and the two control-loop wrappers' `propagate_horizon` / `horizon_gradient`."""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from serving_bits import compare, digest  # noqa: E402

OUT = sys.stdout
GRAD = ("traj", "Sigma", "dU", "dx0", "dSigma0")


def line(tag, a):
    print(tag, digest(a), file=OUT)


def staged(tag, got):
    line(f"{tag} traj", got[0])
    line(f"{tag} Sigma", got[1])
    for k in sorted(got[2]):
        line(f"{tag} {k}", got[2][k])


def horizons(c, nx):
    """(tag, x0, U, keyword arguments) of every variant of a case: R = 1 and 5, the noise level, the start covariance"""
    from test_propagate_host import rollouts, spd
    S0, Q = spd(nx)
    for R in (1, 5):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        for noisy in (False, True):
            for spd_tag, kw in (("Sigma0=0", {}), ("SPD", dict(Sigma0=S0, process_noise=Q))):
                yield f"R={R} noise={noisy} {spd_tag}", x0, U, dict(var_includes_noise=noisy, **kw)


def linear(tag, gp, c, lin, kw0):
    """orders 1 and 2 with the stages, and the gradient chain with the seed gS and without"""
    from test_propagate_grad_host import seeds
    nx = lin.shape[0]
    for what, x0, U, kw in horizons(c, nx):
        for order in (1, 2):
            staged(f"{tag} {what} order={order}", gp.propagate(x0, U, lin, return_stages=True, order=order, **kw, **kw0))
        gx, gS = seeds(x0.shape[0], U.shape[1], nx)
        for s in (None, gS):
            got = gp.propagate_gradient(x0, U, lin, gx, s, **kw, **kw0)
            for k, a in zip(GRAD, got):
                line(f"{tag} {what} grad gS={s is not None} {k}", a)
    # the shorthand shapes (one start row, one control sequence), two results
    for k, a in zip(GRAD, gp.propagate(c["x0"][0], c["U"], lin, **kw0)):
        line(f"{tag} shorthand {k}", a)


def moment(tag, gp, c, lin, kw0):
    from test_propagate_host import rollouts, spd
    nx = lin.shape[0]
    S0, Q = spd(nx)
    for R in (1, 5, 17, 32):
        x0, U = rollouts(c["x0"][0], c["U"] if R <= 5 else c["U"][:4], R)
        Xq = np.ascontiguousarray(np.concatenate([x0, U[:, 0]], axis=1))
        S = np.stack([S0 * (0.05 + 0.01 * r) for r in range(R)])
        for noisy in (False, True):
            for k, a in zip(("mean", "cov", "xcov"), gp.predict_moments(Xq, S, var_includes_noise=noisy, **kw0.get("pm", {}))):
                line(f"{tag} predict_moments R={R} noise={noisy} {k}", a)
            staged(f"{tag} moment R={R} noise={noisy} Sigma0=0",
                   gp.propagate(x0, U, lin, var_includes_noise=noisy, return_stages=True, method="moment", **kw0.get("pg", {})))
        staged(f"{tag} moment R={R} SPD", gp.propagate(x0, U, lin, Sigma0=0.05 * S0, process_noise=Q, return_stages=True,
                                                       method="moment", **kw0.get("pg", {})))


def wrappers():
    import test_gpu_axis_paths as A
    from test_gpu_paths import case
    from test_propagate_grad_host import seeds
    from test_propagate_host import spd
    from unmanned_aerial_vehicles_amd import PreTrainedGP, SimpleQuadrotorGP
    c, gp, _, _ = case("csv")
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = gp, True
    state, Ug = c["x0"][0], np.ascontiguousarray(c["U"].T)
    S0, Q = spd(6)
    gx, gS = seeds(1, Ug.shape[1], 6)
    c2, bg, _, _ = A.case("csv")
    pg = PreTrainedGP("/nonexistent/model.pkl")
    assert pg.load_dict(A.trainer_dict(c2, bg, list(range(6))))
    for name, w, st, U in (("SimpleQuadrotorGP", sq, state, Ug), ("PreTrainedGP", pg, c2["x0"][0], np.ascontiguousarray(c2["U"].T))):
        for order, method in ((1, "linear"), (2, "linear"), (1, "moment")):
            for k, a in zip(("X", "Sigma"), w.propagate_horizon(st, U, 0.1, Sigma0=0.05 * S0, process_noise=Q, order=order,
                                                                 method=method)):
                line(f"{name}.propagate_horizon order={order} method={method} {k}", a)
        for k, a in zip(("X", "Sigma", "dU", "dx0"), w.horizon_gradient(st, U, 0.1, gx[:, 0], gS[:, 0])):
            line(f"{name}.horizon_gradient {k}", a)


def run():
    import test_gpu_axis_propagate as AX
    import test_gpu_moments as MM
    import test_gpu_sparse_propagate as SP
    from test_gpu_paths import case
    from test_gpu_propagate import CASE_NAMES
    from test_sparse_propagate_host import PROBLEMS, problem
    for name in CASE_NAMES:
        c, gp, _, _ = case(name)
        linear(f"exact {name}", gp, c, c["lin"], {})
    for name in CASE_NAMES + ("big", "wide"):
        c, gp, _ = MM.problem(name)
        moment(f"exact {name}", gp, c, c["lin"], {})
    for name in ("a", "csv", "csv345", "gap", "one", "eight"):
        c, bg, _, kw = AX.problem(name)
        linear(f"batch {name}", bg, c, c["lin"], kw)
        pm = dict(in_scaler=kw["in_scaler"], out_scaler=kw["out_scaler"])
        if c["lin"].shape[0] == len(bg.models):      # (predict_moments: the state is the models' own outputs)
            moment(f"batch {name}", bg, c, c["lin"], {"pm": pm, "pg": kw})
    for name in PROBLEMS:
        c, _, kw, _ = problem(name)
        linear(f"sparse {name}", SP.served(name), c, c["lin"], dict(route="chain", **kw))
    wrappers()


KINDS = (" order=1 ", " order=2 ", " grad ", " moment ", " predict_moments ", " shorthand ")


def condense(path):
    """One SHA-256 line per (model, chain) of a full output - over its result lines in order, their count in the tag - for a
    record that is read by people: two full outputs are equal where the condensed ones are (and --compare names the lines)."""
    import hashlib
    groups = {}
    for ln in open(path).read().splitlines():
        tag = ln.rsplit(" ", 1)[0]
        words = tag.split(" ")
        kind = next((k.strip() for k in KINDS if k in tag + " "), None)
        key = words[0] if kind is None or "." in words[0] else " ".join(words[:2]) + " " + kind      # (a wrapper: its method)
        groups.setdefault(key, []).append(ln)
    for key, lines in groups.items():
        print(f"{key} ({len(lines)} results)", hashlib.sha256("\n".join(lines).encode()).hexdigest())


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 3 and sys.argv[1] == "--condense":
        sys.exit(condense(sys.argv[2]))
    with contextlib.redirect_stdout(sys.stderr):      # (what the models print while they load goes to stderr)
        run()
