"""The gradient through exact moment matching on the sparse models (`propagate_moments_gradient`), with and without the tape, in one log.

    python tools/exp_sparse_moments_grad.py [--quick] [--parent-lib build/libgpk_parent.so] [--log profiles/r30_exp_sparse_moments_grad.log]

D = 10, nx = 6, H = 25, Sigma0 = 1e-3 I, R = 1 and 32 rollouts - the problems of tools/exp_sparse_moments.py: one `SparseGP` with P = 6
outputs and six single-output models (`BatchedSparseGP`) at m = 256, 1024 and 4096 inducing inputs.  Wall time per horizon (host clock
around a call that ends in its one synchronisation), median of the repetitions after warm-up, in TWO rounds that alternate the
versions; both rounds are printed: the difference between the rounds of one version is the spread a difference between versions has
to beat.

  tape    `propagate_moments_gradient()`: the one-call chain with every stage's work block kept (5 H + 4 H launches) where the
          horizon's blocks fit option moments_tape_mb (the GPKMT line's `tape` and `launches` are printed);
  plain   the same with moments_tape_mb = 0: the 6 H + 7 H sweep, the engine as the exact classes run it; both must agree bit for
          bit, and the digest of (traj, Sigma, dU, dx0, dSigma0) is printed for each;
  fwd     `propagate_moments()`: the forward chain (5 H launches);
  host    `propagate_moments_gradient(route="host")`: one forward chain and H `predict_moments_vjp` calls.

Exact models: the digest of `propagate_moments_gradient` of the exact classes on the rows of profiles/r29_exp_moments_grad.log (one
model with P = 6 and six per-axis models at N = 1000 and 4096), on this build and, with --parent-lib (a libgpk.so built from the
parent commit, loaded through GPK_LIBRARY in a child process), on the parent's: the exact entries keep their bits.

The lines are printed and appended to --log."""
import argparse
import contextlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from exp_sparse_moments import digest, load_library  # noqa: E402


@contextlib.contextmanager
def stderr_to(path):
    """the process's stderr (the library writes its log lines there) into a file for the duration"""
    sys.stderr.flush()
    saved = os.dup(2)
    with open(path, "w") as f:
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)


def tape_line(be, call):
    """the GPKMT line of one call: (tape, launches, doubles per stage)"""
    with tempfile.NamedTemporaryFile(suffix=".log") as t:
        be.set_options(gram_log=1)
        try:
            with stderr_to(t.name):
                call()
        finally:
            be.set_options(gram_log=0)
        m = re.search(r"^GPKMT tape(\d) h(\d+) stage(\d+) launches(\d+)$", open(t.name).read(), re.M)
    return (int(m.group(1)), int(m.group(4)), int(m.group(3))) if m else (-1, -1, -1)


def exact_rows(say, Ns):
    from exp_propagate import H, NX, horizon, problem
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, WhiteKernel
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    D = 10
    for N in Ns:
        X, Y, lin, rng = problem(N)
        gp = GaussianProcessRegressor(kernel=RBF(2.0) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X, Y)
        X2, Y2, _, _ = problem(N, 1)
        bg = BatchedARDGP(optimizer=None, device=0)
        for b in range(NX):
            k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.roll(np.linspace(1.5, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))
            bg.models.append(GaussianProcessRegressor(kernel=k, alpha=1e-6, normalize_y=True, optimizer=None, device=0).fit(X2, Y2[:, b]))
        S0 = 1e-3 * np.eye(NX)
        seeds = np.random.default_rng(29)
        for tag, model in (("one model P = 6", gp), ("six per-axis models", bg)):
            for R in (1, 32):
                x0, U = horizon(rng, R)
                gx, gS = seeds.standard_normal((H + 1, R, NX)), seeds.standard_normal((H + 1, R, NX, NX))
                a = model.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0)
                say(f"{tag}, N = {N:5d}, R = {R:2d}, H = {H}: digest {digest(*a)}")


def sparse_rows(say, ms, reps):
    for m in ms:
        try:
            sparse_rows_at(say, m, reps)
        except Exception as e:  # noqa: BLE001 - the other sizes are still worth their rows
            say(f"m = {m}: not measured ({type(e).__name__}: {e})")


def sparse_rows_at(say, m, reps):
    from exp_propagate import H, NX, horizon, problem, relerr, wall_us
    from unmanned_aerial_vehicles_amd import RBF, BatchedSparseGP, ConstantKernel, SparseGP, WhiteKernel
    D = 10
    n = 8192 if m >= 4096 else 4096
    X, Y, lin, rng = problem(n)
    Z = X[rng.permutation(n)[:m]] + 0.05 * rng.standard_normal((m, D))
    sp = SparseGP(RBF(2.0) + WhiteKernel(0.05), Z, alpha=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0), device=0).fit(X, Y)
    X2, Y2, _, rng2 = problem(n, 1)
    models = []
    for b in range(NX):
        k = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.roll(np.linspace(1.5, 3.0, D), b)) + WhiteKernel(0.02 * (b + 1))
        Zb = X2[rng2.permutation(n)[:m]] + 0.05 * rng2.standard_normal((m, D))
        models.append(SparseGP(k, Zb, alpha=1e-6, y_mean=Y2[:, b].mean(), y_std=Y2[:, b].std(), device=0).fit(X2, Y2[:, b]))
    bg = BatchedSparseGP(models)
    S0 = 1e-3 * np.eye(NX)
    seeds = np.random.default_rng(30)
    for tag, model, be in (("one sparse model P = 6", sp, sp._backend()), ("six sparse models", bg, models[0]._backend())):
        for R in (1, 32):
            x0, U = horizon(rng, R)
            gx, gS = seeds.standard_normal((H + 1, R, NX)), seeds.standard_normal((H + 1, R, NX, NX))
            grad = lambda: model.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0)                   # noqa: E731
            host = lambda: model.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, route="host")     # noqa: E731
            fwd = lambda: model.propagate_moments(x0, U, lin, Sigma0=S0)                                      # noqa: E731

            def plain():
                be.set_options(moments_tape_mb=0)
                try:
                    return grad()
                finally:
                    be.set_options(moments_tape_mb=1024)

            a, b, c = grad(), plain(), host()
            assert all(np.isfinite(x).all() for x in a)
            same = all(np.array_equal(x, y) for x, y in zip(a, b))
            agree = max(relerr(a[k], c[k]) for k in (2, 3, 4))
            taped, launches, stage = tape_line(be, grad)
            heavy = m >= 4096 or (R == 32 and m >= 1024)
            r = max(3, reps // (8 if heavy else 1))
            t = [[wall_us(f, r if f is not host else max(3, r // 4), warm=1)[0] for f in (grad, plain, fwd, host)] for _ in range(2)]
            best = [min(t[0][j], t[1][j]) for j in range(4)]
            spread = max(abs(t[0][j] - t[1][j]) for j in (0, 1))
            say(f"{tag}, m = {m:4d}, R = {R:2d}, H = {H}: tape{taped} launches {launches} stage {8e-6 * stage:7.2f} MB   "
                f"tape {t[0][0]:10.1f} / {t[1][0]:10.1f} us   plain {t[0][1]:10.1f} / {t[1][1]:10.1f} us   plain / tape {best[1] / best[0]:5.3f}   "
                f"spread {spread:8.1f} us   fwd {t[0][2]:10.1f} / {t[1][2]:10.1f} us   tape / fwd {best[0] / best[2]:5.2f}   "
                f"host {t[0][3]:10.1f} / {t[1][3]:10.1f} us   host / tape {best[3] / best[0]:5.2f}   digest tape {digest(*a)} plain {digest(*b)} "
                f"{'equal' if same else 'DIFFERENT'}   routes agree to {agree:.1e}   [{r} calls per round]")


def child(a):
    load_library()
    say = lambda s: print("ROW " + s, flush=True)      # noqa: E731
    if a.child == "exact":
        exact_rows(say, (1000,) if a.quick else (1000, 4096))
    else:
        sparse_rows(say, (256,) if a.quick else (256, 1024, 4096), a.reps)


def run_child(kind, a, library=None):
    env = dict(os.environ)
    env.pop("GPK_LIBRARY", None)
    if library:
        env["GPK_LIBRARY"] = library
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1100)
    if r.returncode != 0:
        raise RuntimeError(f"{kind} rows failed ({r.returncode}):\n{r.stdout[-3000:]}")
    return [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="m = 256 and N = 1000 only")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--child", choices=("exact", "sparse"), help="(internal) run one block of rows in this process")
    ap.add_argument("--parent-lib", help="a libgpk.so built from the parent commit: the exact digests are taken on it as well")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r30_exp_sparse_moments_grad.log"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/exp_sparse_moments_grad.py on {torch.cuda.get_device_name(0)}; fp64; D = 10, nx = 6, H = 25, Sigma0 = 1e-3 I; wall time "
        f"per horizon, median of up to {a.reps} calls after warm-up; two alternating rounds of every version, both printed (round 1 / round 2)")
    say("# sparse models: tape = propagate_moments_gradient (5 H + 4 H launches within moments_tape_mb), plain = the same with "
        "moments_tape_mb = 0 (6 H + 7 H), fwd = propagate_moments, host = route='host'; spread = the largest difference between the two "
        "rounds of tape or of plain")
    for line in run_child("sparse", a):
        say(line)
    say("# exact models, propagate_moments_gradient: the rows of r29_exp_moments_grad.log, digests of (traj, Sigma, dU, dx0, dSigma0) on "
        "this build" + (" and on the parent commit's" if a.parent_lib else ""))
    for who, library in (("parent", a.parent_lib), ("this  ", None)):
        if who == "parent" and not a.parent_lib:
            continue
        for line in run_child("exact", a, os.path.abspath(library) if library else None):
            say(f"{who}: {line}")
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
