#!/usr/bin/env python3
"""SHA-256 of everything the six one-call serving entries return (gpk_predict_host, _host_multi, _host_cov, _host_grad,
_host_multi_grad, _host_multi_cov) on seeded inputs: one line per entry, model, row count, request and small_path setting.  Two builds of the
library compute the same bits exactly when the two outputs are equal:
    python tools/serving_bits.py > new.txt;  GPK_LIBRARY=/path/to/other/libgpk.so python tools/serving_bits.py > old.txt
    python tools/serving_bits.py --compare old.txt new.txt
Models (N, D, P): (200, 3, 2) - Np = 256: the first row blocks have fewer 64-wide k-chunks than waves - and (1000, 10, 6) -
Np = 1024: four row chunks in small_wtv_grad_kernel; per-axis batches of B = 1, 6, 8 single-output ARD models on the same two
training sets."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

MODELS = ((200, 3, 2), (1000, 10, 6))
ROWS = (1, 16, 17, 32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fit(X, Y, ls):
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor, RBF, WhiteKernel
    gp = GaussianProcessRegressor(kernel=RBF(ls) + WhiteKernel(0.05), alpha=1e-6, normalize_y=True, optimizer=None, device=0)
    gp.fit(X, Y)
    gp.predict(X[:1])
    comp = gp.kernel_.components()
    return gp, comp.sf2 + comp.noise, comp.noise


def multi_args(gps):
    """Argument block of the per-axis entries for single-output models on one training-set size."""
    devs = [g._dev for g, _, _ in gps]
    B = len(devs)
    vp = C.c_void_p * B
    Ws = [d.inverse_factor(False) for d in devs]
    import torch
    torch.cuda.synchronize()
    return {"B": B, "d0": devs[0], "keep": (devs, Ws), "X": vp(*[d.X.data_ptr() for d in devs]),
            "alpha": vp(*[d.alpha.data_ptr() for d in devs]), "W": vp(*[w.data_ptr() for w in Ws]),
            "ls": np.ascontiguousarray(np.stack([d.ls for d in devs])),
            "sf2": np.ascontiguousarray([d.sf2 for d in devs], dtype=np.float64),
            "ym": np.ascontiguousarray([g._y_train_mean[0] for g, _, _ in gps], dtype=np.float64),
            "ys": np.ascontiguousarray([g._y_train_std[0] for g, _, _ in gps], dtype=np.float64),
            "kss": np.ascontiguousarray([k for _, k, _ in gps], dtype=np.float64),
            "noise": np.ascontiguousarray([n for _, _, n in gps], dtype=np.float64)}


def multi(a, Xq, want_var, grad):
    B, d0 = a["B"], a["d0"]
    M, D = Xq.shape
    be = d0.be
    mean, var = np.empty((B, M)), np.empty((B, M)) if want_var else None
    p = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
    head = (be.h, B, a["X"], a["alpha"], d0.N, D, p(a["ls"]), p(a["sf2"]), p(a["ym"]), p(a["ys"]), a["W"] if want_var else None,
            d0.Np, d0.Np, p(a["kss"]), 0.0, p(Xq), M, p(mean), p(var))
    with be.lock:
        be.bind_stream()
        if not grad:
            be.check(be.lib.gpk_predict_host_multi(*head))
            return mean, var
        dmean, dvar = np.empty((B, M, D)), np.empty((B, M, D)) if want_var else None
        be.check(be.lib.gpk_predict_host_multi_grad(*head, p(dmean), p(dvar)))
        return mean, var, dmean, dvar


def multi_cov(a, Xq):
    B, d0 = a["B"], a["d0"]
    M, D = Xq.shape
    be = d0.be
    mean, cov = np.empty((B, M)), np.empty((B, M, M))
    with be.lock:
        be.bind_stream()
        be.check(be.lib.gpk_predict_host_multi_cov(be.h, B, a["X"], a["alpha"], d0.N, D, a["ls"].ctypes.data, a["sf2"].ctypes.data,
                                                   a["ym"].ctypes.data, a["ys"].ctypes.data, a["W"], d0.Np, d0.Np,
                                                   a["noise"].ctypes.data, Xq.ctypes.data, M, mean.ctypes.data, cov.ctypes.data))
    return mean, cov


def run():
    for N, D, P in MODELS:
        rng = np.random.default_rng(N)
        X = rng.standard_normal((N, D))
        Y = np.sin(X @ rng.standard_normal((D, 8))) + 0.1 * rng.standard_normal((N, 8))
        gp, kss, noise = fit(X, Y[:, :P], 1.6)
        dev, ym, ys = gp._dev, gp._y_train_mean, gp._y_train_std
        axis = [fit(X, Y[:, [b]], 1.2 + 0.1 * b + 0.05 * np.arange(D)) for b in range(8)]
        batches = {B: multi_args(axis[:B]) for B in (1, 6, 8)}
        Q = 1.1 * rng.standard_normal((200, D))
        Q[:3] = X[:3]                       # queries at training points: variances near the noise level
        for sp in (1, 0):
            dev.be.set_options(small_path=sp)
            tag = f"N={N} D={D} P={P} small_path={sp}"
            for M in ROWS + (33, 64, 65):
                for v in (None, kss):
                    print(f"predict_host {tag} M={M} var={v is not None}", digest(*dev.predict_host(Q[:M], ym, ys, v, 0.0)))
            for M in ROWS + (33, 200):
                print(f"predict_host_cov {tag} M={M}", digest(*dev.predict_cov_host(Q[:M], ym, ys, noise)))
                for v in (None, kss):
                    print(f"predict_host_grad {tag} M={M} var={v is not None}",
                          digest(*dev.predict_grad_host(Q[:M], ym, ys, v, 0.0)))
            for B, a in batches.items():
                for M in ROWS:
                    for v in (False, True):
                        print(f"predict_host_multi {tag} B={B} M={M} var={v}", digest(*multi(a, Q[:M], v, False)))
                        print(f"predict_host_multi_grad {tag} B={B} M={M} var={v}", digest(*multi(a, Q[:M], v, True)))
                    print(f"predict_host_multi_cov {tag} B={B} M={M}", digest(*multi_cov(a, Q[:M])))
        dev.be.set_options(small_path=1)


def compare(old, new):
    a, b = (dict(line.rsplit(" ", 1) for line in open(f).read().splitlines() if line) for f in (old, new))
    bad = sorted(k for k in a if a[k] != b.get(k))
    for k in sorted(a):
        print(("DIFFERENT " if k in bad else "equal     ") + k, a[k][:16], b.get(k, "missing")[:16])
    only_new = sorted(k for k in b if k not in a)
    for k in only_new:
        print("new only  " + k, b[k][:16])
    print(f"{len(a)} digests of the old build, {len(bad)} different; {len(only_new)} lines only the new build prints")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run()
