"""Measurements of the FITC sparse GP ("FITC"): the weighted statistics pass gpk_sparse_accumulate_fitc and the
FITC posterior against the DTC one.

    python tools/exp_sparse_fitc.py [--quick] [--only cost,csv,plain] [--parent-lib PATH] [--log profiles/r31_exp_sparse_fitc.log]

Every step runs in a process of its own under its own time limit; a step that fails or runs out of time ends the run.  Every
line goes to stdout and is appended to --log.

a. cost: 262 144 rows at D = 9, P = 3, m = 256 / 1024 / 4096 (the sizes of profiles/r11_exp_sparse.log), device pointers, HIP
   events around the whole call, warmed, rounds that alternate: the plain pass (gpk_sparse_accumulate), the weighted pass with the
   fused q_i route, the weighted pass with fitc_fused = 0, and gpk_predict_var_inv alone over the same panels.  The weighted pass
   does N m^2 flops for the lower F^T F and N m^2 for Wuu F^T (Wuu lower triangular): its rate is given as a share of the 78.6 TF
   fp64 matrix peak.  Wuu: NumPy's inverse Cholesky factor of Kuu + 1e-6 I.
b. csv: tools/exp_sparse_select.py's protocol on tests/golden/csv_170501.npz (output 0, 800 rows to train, 200 held out): with
   the exact fit's hyper-parameters, m = 128 / 256 / 512, random and greedy Z, the rms distance of the DTC and of the FITC mean
   and standard deviation from the exact model's on the held-out rows, in std(y).
c. plain: the plain pass must be what it was.  With --parent-lib (a build of the parent commit, GPK_LIBRARY): the digests of
   tools/sparse_serving_bits.py under both libraries, and the plain pass's time under each in alternating processes.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

STEP_LIMIT_S = {"cost": 420, "csv": 420, "plain": 700, "plain_child": 150}
PEAK_TF = 78.6
SIZES = (256, 1024, 4096)
LOG = [None]


def say(line):
    print(line, flush=True)
    if LOG[0]:
        with open(LOG[0], "a") as f:
            f.write(line + "\n")


def mmm(ts):
    return f"{np.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def rbf(A, B, ls):
    a, b = A / ls, B / ls
    d2 = np.sum(a * a, axis=1)[:, None] + np.sum(b * b, axis=1)[None, :] - 2.0 * a @ b.T
    return np.exp(-0.5 * np.maximum(d2, 0.0))


def problem(m, N, D=9, P=3):
    rng = np.random.default_rng(m)
    X, Yn, Z = rng.standard_normal((N, D)), rng.standard_normal((N, P)), rng.standard_normal((m, D))
    ls = np.ascontiguousarray(2.0 * (1.0 + 0.05 * np.arange(D)))
    return X, Yn, Z, ls


def panel_rows(mp):
    rows = (128 << 20) // ((mp + 128) * 8) // 256 * 256
    return max(1024, min(16384, rows))


def cost(quick):
    import torch
    from scipy.linalg import cholesky, solve_triangular
    from exp_sparse import dev_ms
    from unmanned_aerial_vehicles_amd import _lib
    from unmanned_aerial_vehicles_amd.device import Backend
    D, P, s2 = 9, 3, 0.01
    N = 32768 if quick else 262144
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for m in SIZES:
        be = Backend(0)
        X, Yn, Z, ls = problem(m, N)
        lsp = ls.ctypes.data_as(C.POINTER(C.c_double))
        mp = (m + 127) // 128 * 128
        nt = mp + 128
        W = np.eye(mp)
        W[:m, :m] = solve_triangular(cholesky(rbf(Z, Z, ls) + 1e-6 * np.eye(m), lower=True), np.eye(m), lower=True)
        dX, dY, dZ, dW = be.upload(X), be.upload(Yn), be.upload(Z), be.upload(W)
        S = torch.zeros((nt, nt), dtype=torch.float64, device=be.device)
        lam = torch.zeros((1,), dtype=torch.float64, device=be.device)
        panel = panel_rows(mp)
        work = torch.empty(((panel + 127) // 128 * 128, mp), dtype=torch.float64, device=be.device)
        var = torch.empty((panel + 128,), dtype=torch.float64, device=be.device)
        lib, h = be.lib, be.h

        def plain():
            be.check(lib.gpk_sparse_accumulate(h, p(dX), p(dY), N, p(dZ), m, D, P, lsp, 1.0, p(S), nt))

        def weighted():
            be.check(lib.gpk_sparse_accumulate_fitc(h, p(dX), p(dY), N, p(dZ), m, D, P, lsp, 1.0, p(S), nt, p(dW), mp, s2, p(lam), None))

        def fused():
            be.set_options(fitc_fused=1)
            weighted()

        def unfused():
            be.set_options(fitc_fused=0)
            weighted()

        def var_inv():
            for r0 in range(0, N, panel):
                n = min(panel, N - r0)
                be.check(lib.gpk_predict_var_inv(h, _lib.GPK_F64, p(dZ), m, D, lsp, 1.0, p(dW), mp, mp, p(dX[r0:]), n, 1.0, -1e300,
                                                 p(work), p(var)))

        routes = (("plain", plain), ("fused", fused), ("fitc_fused=0", unfused), ("var_inv", var_inv))
        with be.lock:
            be.bind_stream()
            for _, f in routes:      # warm-up: code objects, the work area's pages
                f()
            be.sync()
            S.zero_(), lam.zero_()
            fused()
            be.sync()
            Sf, lf = S.clone(), float(lam.cpu()[0])
            S.zero_(), lam.zero_()
            unfused()
            be.sync()
            same = bool(torch.equal(S, Sf)) and float(lam.cpu()[0]) == lf
            ts = {k: [] for k, _ in routes}
            for _ in range(3 if m == 4096 else 7):
                for k, f in routes:
                    ts[k].append(dev_ms(f))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        fl = 2.0 * N * m * m
        say(f"cost m = {m:5d} N = {N} panel = {panel}: plain {mmm(ts['plain'])}   weighted, fused {mmm(ts['fused'])} = "
            f"{fl / med['fused'] / 1e9:5.1f} TF ({100 * fl / med['fused'] / 1e9 / PEAK_TF:4.1f} % of the fp64 matrix peak)   "
            f"weighted, fitc_fused=0 {mmm(ts['fitc_fused=0'])}   gpk_predict_var_inv alone {mmm(ts['var_inv'])}")
        say(f"     m = {m:5d} weighted / plain {med['fused'] / med['plain']:5.2f}   fused / unfused {med['fused'] / med['fitc_fused=0']:5.2f}   "
            f"fused against plain + var_inv {med['fused'] / (med['plain'] + med['var_inv']):5.2f}"
            f"{'   (EXCEEDS the sum)' if med['fused'] > med['plain'] + med['var_inv'] else ''}   fused and unfused give the same bits: {same}")
        be.lib.gpk_destroy(be.h)
        del dX, dY, dW, work, S
        torch.cuda.empty_cache()


def csv():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, SparseGP, WhiteKernel
    d = np.load(os.path.join(os.path.dirname(HERE), "tests", "golden", "csv_170501.npz"))
    X, Y = d["X10"], d["Y6"]
    sx = X.std(axis=0)
    X = (X - X.mean(axis=0)) / np.where(sx > 0, sx, 1.0)
    Xt, yt, Xh, yh = X[:800], Y[:800, 0], X[800:], Y[800:, 0]
    kern = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(np.ones(X.shape[1]), (0.1, 100.0)) + WhiteKernel(0.1, (1e-5, 10.0))
    ex = GaussianProcessRegressor(kernel=kern, alpha=1e-6, normalize_y=True, device=0).fit(Xt, yt)
    em, es = ex.predict(Xh, return_std=True)
    sd = yt.std()
    say(f"csv: exact fit on 800 rows of csv_170501 (output 0), kernel {ex.kernel_}, LML {ex.log_marginal_likelihood_value_:.3f}, "
        f"rms error on the 200 held-out rows {np.sqrt(np.mean((em - yh) ** 2)) / sd:.3f} std(y)")
    rms = lambda a: float(np.sqrt(np.mean(a ** 2)) / sd)  # noqa: E731
    for m in (128, 256, 512):
        for sel in ("random", "greedy"):
            out = {}
            for kind in ("dtc", "fitc"):
                sp = SparseGP.from_exact(ex, inducing=m, random_state=0, selection=sel, approximation=kind).partial_fit(Xt, yt)
                sm, ss = sp.predict(Xh, return_std=True)
                out[kind] = (rms(sm - em), rms(ss - es), rms(sm - yh), sp.bound())
            a, b = out["dtc"], out["fitc"]
            say(f"csv m = {m:3d} {sel:<6s} Z: rms |mean - exact| / std(y)  DTC {a[0]:.3e}  FITC {b[0]:.3e}   rms |std - exact| / std(y)  DTC "
                f"{a[1]:.3e}  FITC {b[1]:.3e}   FITC closer: mean {b[0] < a[0]}, std {b[1] < a[1]}   rms error on the held-out rows  DTC "
                f"{a[2]:.3f}  FITC {b[2]:.3f}   DTC bound {a[3]:.3f}  FITC likelihood {b[3]:.3f}")


def plain_child(quick):
    """the plain pass's time under the library GPK_LIBRARY names (or this build): one line per m.  Plain ctypes on the C ABI, as
    tools/sparse_serving_bits.py: an older build lacks the entries the package binds."""
    import torch
    from exp_sparse import dev_ms
    from unmanned_aerial_vehicles_amd._build import LIB_PATH
    lib = C.CDLL(os.environ.get("GPK_LIBRARY") or LIB_PATH)      # (torch first: one HIP runtime in the process)
    vp, i64, dp = C.c_void_p, C.c_int64, C.POINTER(C.c_double)
    lib.gpk_create.argtypes, lib.gpk_set_stream.argtypes, lib.gpk_destroy.argtypes = [C.POINTER(vp), C.c_int], [vp, vp], [vp]
    lib.gpk_destroy.restype = None
    lib.gpk_sparse_accumulate.argtypes = [vp, vp, vp, i64, vp, i64, C.c_int, C.c_int, dp, C.c_double, vp, i64]
    D, P = 9, 3
    N = 32768 if quick else 262144
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for m in SIZES:
        h = vp()
        assert lib.gpk_create(C.byref(h), 0) == 0
        assert lib.gpk_set_stream(h, torch.cuda.current_stream(dev).cuda_stream) == 0
        X, Yn, Z, ls = problem(m, N)
        lsp = ls.ctypes.data_as(dp)
        nt = (m + 127) // 128 * 128 + 128
        dX, dY, dZ = (torch.from_numpy(a).to(dev) for a in (X, Yn, Z))
        S = torch.zeros((nt, nt), dtype=torch.float64, device=dev)

        def run():
            assert lib.gpk_sparse_accumulate(h, p(dX), p(dY), N, p(dZ), m, D, P, lsp, 1.0, p(S), nt) == 0

        run(), run()
        torch.cuda.synchronize()
        ts = [dev_ms(run) for _ in range(3 if m == 4096 else 9)]
        say(f"plain pass under {os.environ.get('GPK_LIBRARY', 'this build')}: m = {m:5d} N = {N}: {mmm(ts)}")
        lib.gpk_destroy(h)
        del dX, dY, S
        torch.cuda.empty_cache()


def plain(quick, parent, log):
    if not parent or not os.path.exists(parent):
        say("plain: no --parent-lib given (a build of the parent commit): step skipped")
        return 0
    bits = os.path.join(HERE, "sparse_serving_bits.py")
    outs = []
    for lib in (None, parent):
        env = dict(os.environ)
        env.pop("GPK_LIBRARY", None)
        if lib:
            env["GPK_LIBRARY"] = lib
        r = subprocess.run([sys.executable, bits], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=200, env=env)
        if r.returncode != 0:
            say(f"plain: sparse_serving_bits.py failed under {lib or 'this build'}: {r.stderr[-300:]}")
            return r.returncode
        outs.append(r.stdout.splitlines())
    common = min(len(outs[0]), len(outs[1]))
    same = sum(a == b for a, b in zip(outs[0], outs[1]))
    say(f"plain: sparse_serving_bits.py digests, this build {len(outs[0])} lines, parent build {len(outs[1])} lines: {same} of {common} equal"
        f"{'' if same == common == len(outs[0]) == len(outs[1]) else '   (DIFFERENT)'}")
    for rnd in range(2):
        for lib in (None, parent):
            env = dict(os.environ)
            env.pop("GPK_LIBRARY", None)
            if lib:
                env["GPK_LIBRARY"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "plain_child"] + (["--quick"] if quick else []) + (["--log", log] if log else [])
            rc = subprocess.run(cmd, timeout=STEP_LIMIT_S["plain_child"], env=env).returncode
            if rc != 0:
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer rows")
    ap.add_argument("--only", default="cost,csv,plain")
    ap.add_argument("--parent-lib", default=None, help="libgpk.so built from the parent commit")
    ap.add_argument("--log", default=None, help="append every line to this file")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    a = ap.parse_args()
    LOG[0] = a.log
    if a.step is None:
        say("# tools/exp_sparse_fitc.py; fp64")
        for step in a.only.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--quick"] if a.quick else [])
            cmd += (["--log", a.log] if a.log else []) + (["--parent-lib", a.parent_lib] if a.parent_lib else [])
            try:
                rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
            except subprocess.TimeoutExpired:
                say(f"step {step}: no result within {STEP_LIMIT_S[step]} s - stopping here")
                return 124
            if rc != 0:
                say(f"step {step}: exit status {rc} - stopping here")
                return rc
        return 0
    if a.step == "plain":
        return plain(a.quick, a.parent_lib, a.log)
    import torch
    say(f"## {a.step} on {torch.cuda.get_device_name(0)}")
    {"cost": lambda: cost(a.quick), "csv": csv, "plain_child": lambda: plain_child(a.quick)}[a.step]()
    return 0


if __name__ == "__main__":
    sys.exit(main())
