"""Exact moment matching on the sparse models (K11, `propagate_moments`), and the query dimension of the pair launch, in one log.

    python tools/exp_sparse_moments.py [--quick] [--parent-lib build/libgpk_parent.so] [--log profiles/r28_exp_sparse_moments.log]

D = 10, nx = 6, H = 25, R = 1 and 32 rollouts - the problems of tools/exp_moments.py.  Wall time per horizon (host clock around a
call that ends in its one synchronisation), median of the repetitions after warm-up.  Every comparison of two versions is taken
in rounds that alternate them, and every round is printed: the difference between rounds of one version is the spread a difference
between versions has to beat.

Sparse models: one `SparseGP` with P = 6 outputs and six single-output models (`BatchedSparseGP`), m = 256, 1024 and 4096 inducing
inputs on n = 4096 rows (8192 for m = 4096):

  mm     `propagate_moments()`: the one-call chain (5 H launches) with the pair launch's default groups of queries;
  mm1    the same with option moments_query_groups = 1: the launch without the query dimension (where the default already is one
         group - 512 workgroups or more, or R = 1 - the column repeats mm); both must agree bit for bit;
  lin    `propagate(route="chain")`: the sparse first-order chain (3 H launches);
  fin    the finishing launch of a stage alone (event bracket GPK_TIMED_PROPAGATE).

Exact models: the rows of profiles/r27_exp_moments.log - `propagate(method="moment")` of one model with P = 6 and of six per-axis
models at N = 1000 and 4096 - on this build and, with --parent-lib (a libgpk.so built from the parent commit, loaded through
GPK_LIBRARY in a child process), on the parent's, alternating; a digest of traj and Sigma shows that the bits are the same.

The lines are printed and appended to --log."""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:12]


def load_library():
    """The package on whatever GPK_LIBRARY names: a parent build lacks this change's entries, which are then left unbound."""
    import torch  # noqa: F401  (its HIP runtime first, as _lib.load does)
    from unmanned_aerial_vehicles_amd import _lib
    path = os.environ.get("GPK_LIBRARY")
    if path:
        lib = ctypes.CDLL(path)
        for name in [n for n in _lib.SIGNATURES if not hasattr(lib, n)]:
            del _lib.SIGNATURES[name]
    _lib.load()


def groups_of(m, pairs, R, cus=256):
    """the pair launch's groups of queries (gpk_moments.hip, mm_query_groups) for m rows, `pairs` pairs of models and R queries"""
    nt = -(-m // 64)
    wgs = min(nt * (nt + 1) // 2, 512) * pairs
    return 1 if wgs >= 512 else max(1, min(R, 2 * cus // wgs))


def exact_rows(say, Ns, reps):
    from exp_propagate import H, NX, horizon, problem, wall_us
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
        for tag, model in (("one model P = 6", gp), ("six per-axis models", bg)):
            for R in (1, 32):
                x0, U = horizon(rng, R)
                mm = lambda: model.propagate(x0, U, lin, Sigma0=S0, method="moment")      # noqa: E731
                a = mm()
                t = wall_us(mm, max(3, reps // (8 if R == 32 else 1)), warm=2)
                say(f"{tag}, N = {N:5d}, R = {R:2d}, H = {H}: mm {t[0]:10.1f} us   digest {digest(a[0], a[1])}")


def sparse_rows(say, ms, reps):
    for m in ms:
        try:
            sparse_rows_at(say, m, reps)
        except Exception as e:  # noqa: BLE001 - the other sizes are still worth their rows
            say(f"m = {m}: not measured ({type(e).__name__}: {e})")


def sparse_rows_at(say, m, reps):
    from exp_propagate import H, NX, horizon, problem, wall_us
    from unmanned_aerial_vehicles_amd import RBF, BatchedSparseGP, ConstantKernel, SparseGP, WhiteKernel, _lib
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
    for tag, model, be, pairs in (("one sparse model P = 6", sp, sp._backend(), 1), ("six sparse models", bg, models[0]._backend(), 21)):
        for R in (1, 32):
            x0, U = horizon(rng, R)
            mm = lambda: model.propagate_moments(x0, U, lin, Sigma0=S0)                   # noqa: E731
            first = lambda: model.propagate(x0, U, lin, Sigma0=S0, route="chain")          # noqa: E731
            nq = groups_of(m, pairs, R)
            a = mm()
            assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
            r_mm = max(3, reps // (8 if R == 32 else 1))
            rounds = []
            for _ in range(2):      # alternating: split, one group, split, one group
                t_split = wall_us(mm, r_mm, warm=2)[0]
                if nq > 1:
                    be.set_options(moments_query_groups=1)
                    try:
                        b1 = mm()
                        assert np.array_equal(a[0], b1[0]) and np.array_equal(a[1], b1[1]), "the query split changed bits"
                        t_one = wall_us(mm, r_mm, warm=2)[0]
                    finally:
                        be.set_options(moments_query_groups=0)
                else:
                    t_one = t_split
                rounds.append((t_split, t_one))
            t_lin = wall_us(first, reps)[0]
            be.call("gpk_timing", 1)
            try:
                mm()
                ms_, cnt = np.zeros(64), ctypes.c_int(0)
                be.call("gpk_kernel_times", _lib.GPK_TIMED_PROPAGATE, _lib.host_ptr(ms_), 64, ctypes.byref(cnt))
            finally:
                be.call("gpk_timing", 0)
            fin = 1e3 * float(np.median(ms_[:cnt.value]))
            best = min(r[0] for r in rounds)
            say(f"{tag}, m = {m:4d}, R = {R:2d}, H = {H}: groups {nq:2d}   mm {rounds[0][0]:10.1f} / {rounds[1][0]:10.1f} us   "
                f"mm1 {rounds[0][1]:10.1f} / {rounds[1][1]:10.1f} us   mm1 / mm {min(r[1] for r in rounds) / best:5.2f}   "
                f"lin {t_lin:8.1f} us   mm / lin {best / t_lin:6.1f}   fin {fin:5.1f} us, {cnt.value} brackets")


def child(a):
    load_library()
    say = lambda s: print("ROW " + s, flush=True)      # noqa: E731
    if a.child == "exact":
        exact_rows(say, (1000,) if a.quick else (1000, 4096), a.reps)
    else:
        sparse_rows(say, (256,) if a.quick else (256, 1024, 4096), a.reps)


def run_child(kind, a, library=None):
    env = dict(os.environ)
    env.pop("GPK_LIBRARY", None)
    if library:
        env["GPK_LIBRARY"] = library
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(a.reps)] + (["--quick"] if a.quick else [])
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{kind} rows failed ({r.returncode}):\n{r.stdout[-3000:]}")
    return [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="m = 256 and N = 1000 only")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--child", choices=("exact", "sparse"), help="(internal) run one block of rows in this process")
    ap.add_argument("--parent-lib", help="a libgpk.so built from the parent commit: the exact rows are run on it as well")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r28_exp_sparse_moments.log"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/exp_sparse_moments.py on {torch.cuda.get_device_name(0)}; fp64; D = 10, nx = 6, H = 25, Sigma0 = 1e-3 I; wall time "
        f"per horizon, median of up to {a.reps} calls after warm-up; two alternating rounds per comparison, both printed")
    say("# sparse models: mm = propagate_moments (default groups of queries in the pair launch), mm1 = one group, lin = the sparse "
        "first-order chain")
    for line in run_child("sparse", a):
        say(line)
    say("# exact models, propagate(method='moment'): the rows of r27_exp_moments.log, this build"
        + (" and the parent commit's, alternating" if a.parent_lib else ""))
    for rnd in (1, 2):
        for who, library in (("parent", a.parent_lib), ("this  ", None)):
            if who == "parent" and not a.parent_lib:
                continue
            for line in run_child("exact", a, os.path.abspath(library) if library else None):
                say(f"round {rnd}, {who}: {line}")
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
