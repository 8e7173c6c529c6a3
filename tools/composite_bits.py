#!/usr/bin/env python3
"""SHA-256 of everything the composite C entries return (a whole model behind the handle: gpk_fit / gpk_predict* / gpk_lml /
gpk_export / gpk_import, the per-axis batch gpk_*_batched*, the sparse model gpk_sparse_*) on seeded inputs, through ctypes:
one line per call.  Two builds of the library compute the same bits exactly when their outputs are equal:
    python tools/composite_bits.py [--dump DIR] > new.txt
    GPK_LIBRARY=/path/to/other/libgpk.so python tools/composite_bits.py [--dump DIR] > old.txt
    python tools/composite_bits.py --compare old.txt new.txt
    python tools/composite_bits.py --compare old1.txt old2.txt new1.txt new2.txt
The four-file form takes two runs of each build: a line on which the two OLD runs differ is named, left out of the digest
comparison and compared by value instead (--dump DIR of each run, DIR = the digest file's name + ".d"): the new build may
differ from the first old run by at most twice the old build's own run-to-run difference, element by element; more than one
such line in ten is an error (the inputs are wrong).
    python tools/composite_bits.py --time > t.txt          median / 10th / 90th percentile in us of the serving cells (1000 calls after 200;
                                                           the two-panel cell 300 after 50)
    python tools/composite_bits.py --time-table old1 new1 old2 new2     (runs taken alternately) -> markdown table
A cell passes if both runs of the new build lie inside the old build's two-run range widened on either side by the larger of
the difference of the two old runs and the largest relative old-to-old difference of any cell, applied to this cell."""
import ctypes as C
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

BIG = 16384 + 130            # two query panels, the second ragged
DUMP_MAX_BYTES = 64 << 20    # larger results are compared by digest only
_dump_dir, _line = None, 0


def dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emit(label, *values):
    """One digest line over the arrays / scalars a call returned (None: not requested)."""
    global _line
    arrays = [np.ascontiguousarray(v) for v in values if v is not None]
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    print(label, h.hexdigest(), flush=True)
    if _dump_dir and sum(a.nbytes for a in arrays) <= DUMP_MAX_BYTES:
        np.save(os.path.join(_dump_dir, f"{_line:04d}.npy"), np.concatenate([a.astype(np.float64).ravel() for a in arrays]))
    _line += 1


class Handle:
    def __init__(self, **options):
        from unmanned_aerial_vehicles_amd import _lib
        self.lib, self.h = _lib.load(), C.c_void_p()
        assert self.lib.gpk_create(C.byref(self.h), 0) == 0
        self.ok(self.lib.gpk_set_stream(self.h, C.c_void_p(-1)))
        self.set(**options)

    def set(self, **options):
        for k, v in options.items():
            self.ok(self.lib.gpk_set_option(self.h, k.encode(), v))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"libgpk error {rc}: {self.lib.gpk_last_error(self.h).decode()}")

    def close(self):
        self.lib.gpk_destroy(self.h)

    # -- one model
    def fit(self, X, Y, ls, sf2, noise, jitter):
        ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
        self.ok(self.lib.gpk_fit(self.h, dp(X), X.shape[0], X.shape[1], dp(Y), Y.shape[1], dp(ls), len(ls), sf2, noise, jitter, 1))
        self.D, self.P = X.shape[1], Y.shape[1]

    def predict(self, Q, want_var, vin, dtype=np.float64):
        Q = np.ascontiguousarray(Q, dtype=dtype)
        mean = np.empty((len(Q), self.P), dtype=dtype)
        var = np.empty((len(Q), self.P), dtype=dtype) if want_var else None
        self.ok(self.lib.gpk_predict(self.h, vp(Q), len(Q), vp(mean), vp(var), 1 if dtype == np.float64 else 0, vin))
        return mean, var

    def cov(self, Q):
        mean, cov = np.empty((len(Q), self.P)), np.empty((self.P, len(Q), len(Q)))
        self.ok(self.lib.gpk_predict_model_cov(self.h, dp(Q), len(Q), dp(mean), dp(cov)))
        return mean, cov

    def grad(self, Q, want_var, vin):
        M, P, D = len(Q), self.P, self.D
        mean, dmean = np.empty((M, P)), np.empty((M, P, D))
        var, dvar = (np.empty((M, P)), np.empty((M, P, D))) if want_var else (None, None)
        self.ok(self.lib.gpk_predict_model_grad(self.h, dp(Q), M, dp(mean), dp(var), dp(dmean), dp(dvar), vin))
        return mean, var, dmean, dvar

    def lml(self, theta, want_grad):
        v, g = C.c_double(), np.zeros(len(theta)) if want_grad else None
        self.ok(self.lib.gpk_lml(self.h, dp(theta), 0 if theta is None else len(theta), C.byref(v), dp(g)))
        return np.float64(v.value), g

    def export(self, N):
        L, alpha, ym, ys = np.empty((N, N)), np.empty((N, self.P)), np.empty(self.P), np.empty(self.P)
        n, d, p, lml = C.c_int64(), C.c_int(), C.c_int(), C.c_double()
        self.ok(self.lib.gpk_export(self.h, C.byref(n), C.byref(d), C.byref(p), dp(L), dp(alpha), dp(ym), dp(ys), C.byref(lml)))
        return np.array([n.value, d.value, p.value], dtype=np.float64), L, alpha, ym, ys, np.float64(lml.value)

    # -- the per-axis batch
    def fit_batched(self, X, Y, ls, sf2, noise, jitter):
        self.B, self.D = Y.shape[1], X.shape[1]
        info = (C.c_int * self.B)()
        self.ok(self.lib.gpk_fit_batched(self.h, self.B, dp(X), X.shape[0], self.D, dp(Y), dp(ls), ls.shape[1], dp(sf2), dp(noise),
                                         jitter, 1, info))
        return np.array(list(info), dtype=np.float64)

    def predict_batched(self, Q, want_var, vin):
        mean, var = np.empty((len(Q), self.B)), np.empty((len(Q), self.B)) if want_var else None
        self.ok(self.lib.gpk_predict_batched(self.h, dp(Q), len(Q), dp(mean), dp(var), vin))
        return mean, var

    def grad_batched(self, Q, want_var, vin):
        M, B, D = len(Q), self.B, self.D
        mean, dmean = np.empty((M, B)), np.empty((M, B, D))
        var, dvar = (np.empty((M, B)), np.empty((M, B, D))) if want_var else (None, None)
        self.ok(self.lib.gpk_predict_batched_grad(self.h, dp(Q), M, dp(mean), dp(var), dp(dmean), dp(dvar), vin))
        return mean, var, dmean, dvar

    def cov_batched(self, Q):
        mean, cov = np.empty((len(Q), self.B)), np.empty((self.B, len(Q), len(Q)))
        self.ok(self.lib.gpk_predict_batched_cov(self.h, dp(Q), len(Q), dp(mean), dp(cov)))
        return mean, cov

    def lml_batched(self, thetas, want_grad):
        v, g = np.empty(self.B), np.zeros_like(thetas) if want_grad else None
        self.ok(self.lib.gpk_lml_batched(self.h, dp(thetas), 0 if thetas is None else thetas.shape[1], dp(v), dp(g)))
        return v, g

    # -- the sparse model
    def sparse_begin(self, Z, P, ls, sf2, noise, jitter, jitter_uu, ym, ys):
        self.P = P
        self.ok(self.lib.gpk_sparse_begin(self.h, dp(Z), Z.shape[0], Z.shape[1], P, dp(ls), len(ls), sf2, noise, jitter, jitter_uu,
                                          dp(ym), dp(ys)))

    def sparse_update(self, X, Y):
        self.ok(self.lib.gpk_sparse_update(self.h, dp(np.ascontiguousarray(X)), dp(np.ascontiguousarray(Y)), len(X)))

    def sparse_finalize(self):
        info, bound, n = C.c_int(), C.c_double(), C.c_int64()
        self.ok(self.lib.gpk_sparse_finalize(self.h, C.byref(info)))
        self.ok(self.lib.gpk_sparse_bound(self.h, C.byref(bound), C.byref(n)))
        return np.array([info.value, n.value], dtype=np.float64), np.float64(bound.value)

    def sparse_predict(self, Q, want_var, vin):
        mean, var = np.empty((len(Q), self.P)), np.empty((len(Q), self.P)) if want_var else None
        self.ok(self.lib.gpk_sparse_predict(self.h, dp(Q), len(Q), dp(mean), dp(var), vin))
        return mean, var

    def sparse_grad(self, Q, D):
        M, P = len(Q), self.P
        mean, var, dmean, dvar = np.empty((M, P)), np.empty((M, P)), np.empty((M, P, D)), np.empty((M, P, D))
        self.ok(self.lib.gpk_sparse_predict_grad(self.h, dp(Q), M, dp(mean), dp(var), dp(dmean), dp(dvar), 1))
        return mean, var, dmean, dvar

    def sparse_cov(self, Q):
        mean, cov = np.empty((len(Q), self.P)), np.empty((self.P, len(Q), len(Q)))
        self.ok(self.lib.gpk_sparse_predict_cov(self.h, dp(Q), len(Q), dp(mean), dp(cov)))
        return mean, cov

    def sparse_predict_multi(self, models, Q):
        """Mean and variance of the single-output sparse models behind `models` (Handles), served by this handle."""
        B, handles = len(models), (C.c_void_p * len(models))(*[x.h for x in models])
        mean, var = np.empty((len(Q), B)), np.empty((len(Q), B))
        self.ok(self.lib.gpk_sparse_predict_multi(self.h, B, handles, dp(Q), len(Q), dp(mean), dp(var), 1))
        return mean, var

    def sparse_export(self, m, D, n_ls):
        P = self.P
        Z, G, g, yy = np.empty((m, D)), np.empty((m, m)), np.empty((m, P)), np.empty(P)
        ls, hyper, ym, ys = np.empty(n_ls), np.empty(4), np.empty(P), np.empty(P)
        i64, ints = C.c_int64(), [C.c_int() for _ in range(3)]
        n = C.c_int64()
        self.ok(self.lib.gpk_sparse_export(self.h, C.byref(i64), C.byref(ints[0]), C.byref(ints[1]), C.byref(ints[2]), dp(Z), dp(G),
                                           dp(g), dp(yy), C.byref(n), dp(ls), dp(hyper), dp(ym), dp(ys)))
        return np.array([i64.value, n.value] + [i.value for i in ints], dtype=np.float64), Z, G, g, yy, ls, hyper, ym, ys


def problem(N, D, P, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    Y = np.ascontiguousarray(np.sin(X @ rng.standard_normal((D, P))) + 0.1 * rng.standard_normal((N, P)))
    Q = 1.1 * rng.standard_normal((BIG, D))
    Q[:3] = X[:3]                       # queries at training rows: variances near the noise level (the fp64 recheck of fp32 serving)
    return rng, X, Y, Q


def run_model(N, D, P):
    rng, X, Y, Q = problem(N, D, P, N)
    ls = np.array([1.6]) if D == 3 else 1.2 + 0.05 * np.arange(D)
    sf2, noise, jitter = 1.3, 0.05, 1e-6
    tag = f"N={N} D={D} P={P}"
    h = Handle()
    h.fit(X, Y, ls, sf2, noise, jitter)
    exported = h.export(N)
    emit(f"export {tag}", *exported)
    emit(f"lml {tag} theta=stored", *h.lml(None, False))
    for name, theta in (("fitted", np.log(np.r_[ls, noise])), ("trial", np.log(np.r_[ls, noise]) + rng.uniform(-0.3, 0.3, len(ls) + 1))):
        for g in (False, True):
            emit(f"lml {tag} theta={name} grad={g}", *h.lml(theta, g))
    for M in (1, 32, 33, 64, 65, 300, BIG):
        for v in (False, True):
            for vin in (0, 1):
                emit(f"predict {tag} f64 M={M} var={v} vin={vin}", *h.predict(Q[:M], v, vin))
    for M in (300, BIG):
        emit(f"predict {tag} f32 M={M} var=True vin=1", *h.predict(Q[:M], True, 1, np.float32))
    for M in (32, 300) + ((4200,) if P == 2 else ()):          # 4200 > GPK_HOST_MAX_M: the single-panel route
        emit(f"predict_model_cov {tag} M={M}", *h.cov(Q[:M]))
    for M in (32, 300):
        for v in (False, True):
            emit(f"predict_model_grad {tag} M={M} var={v}", *h.grad(Q[:M], v, 1))
    emit(f"lml {tag} theta=trial grad=True (after serving)", *h.lml(np.log(np.r_[ls, 2 * noise]), True))
    h2 = Handle()
    _, L, alpha, ym, ys, _ = exported
    h2.ok(h2.lib.gpk_import(h2.h, dp(X), N, D, dp(L), dp(alpha), P, dp(ls), len(ls), sf2, noise, dp(ym), dp(ys)))
    h2.D, h2.P = D, P
    emit(f"import+predict {tag} f64 M=33 var=True vin=1", *h2.predict(Q[:33], True, 1))
    h2.close()
    h.close()


def run_gated():
    """The low-noise model of tests/test_gpu_composite.py::test_composite_fp32_predict_is_gated: the fp32 mean gate refuses it."""
    N, D, P, M = 3000, 9, 3, 300
    rng = np.random.default_rng(7)
    X = rng.standard_normal((N, D))
    Y = np.ascontiguousarray(np.sin(X @ rng.standard_normal((D, P))) + 0.1 * rng.standard_normal((N, P)))
    Q = np.ascontiguousarray(np.vstack([X[:100], rng.standard_normal((M - 100, D))]), dtype=np.float32)
    h = Handle()
    h.fit(X, Y, 2.0, 1.0, 1e-3, 1e-8)
    m32, v32 = h.predict(Q, True, 1, np.float32)
    m64, v64 = h.predict(Q.astype(np.float64), True, 1)
    refused = np.array_equal(m32, m64.astype(np.float32)) and np.array_equal(v32, v64.astype(np.float32))
    print(f"# fp32 request on the low-noise model served by the fp64 kernels: {refused}")
    emit(f"predict N={N} D={D} P={P} noise=1e-3 f32 M={M} var=True vin=1 (mean gate)", m32, v32)
    h.close()


def run_batched(N, D, B):
    rng = np.random.default_rng(7 * N + B)
    X = rng.standard_normal((N, D))
    Y = np.ascontiguousarray(np.sin(X @ rng.standard_normal((D, B))) * (1.0 + np.arange(B)) + 0.1 * rng.standard_normal((N, B)))
    ls = np.ascontiguousarray(np.exp(rng.uniform(-0.3, 0.5, (B, D))) * np.sqrt(D) / 1.5)
    sf2 = np.ascontiguousarray(np.exp(rng.uniform(-0.5, 0.5, B)))
    noise = np.ascontiguousarray(np.exp(rng.uniform(np.log(0.01), np.log(0.2), B)))
    Q = 1.1 * rng.standard_normal((BIG, D))
    Q[:3] = X[:3]
    tag = f"N={N} D={D} B={B}"
    h = Handle()
    emit(f"fit_batched {tag} info", h.fit_batched(X, Y, ls, sf2, noise, 1e-6))
    emit(f"lml_batched {tag} theta=stored", *h.lml_batched(None, False))
    fitted = np.ascontiguousarray(np.log(np.c_[ls, noise]))
    for name, th in (("fitted", fitted), ("trial", np.ascontiguousarray(fitted + rng.uniform(-0.3, 0.3, fitted.shape)))):
        for g in (True, False):
            emit(f"lml_batched {tag} theta={name} grad={g}", *h.lml_batched(th, g))
    for M in (25, 33, 700, BIG):
        for v in (False, True):
            for vin in (0, 1):
                emit(f"predict_batched {tag} M={M} var={v} vin={vin}", *h.predict_batched(Q[:M], v, vin))
    for M in (25, 33, 700):
        for v in (False, True):
            emit(f"predict_batched_grad {tag} M={M} var={v}", *h.grad_batched(Q[:M], v, 1))
    for M in (25, 200):
        emit(f"predict_batched_cov {tag} M={M}", *h.cov_batched(Q[:M]))
    h.close()


def run_sparse(m, P):
    D, n = 3, 700 + 333
    rng, X, Y, Q = problem(n, D, P, 100 * m + P)
    Z = np.ascontiguousarray(X[rng.choice(n, m, replace=False)] + 0.01 * rng.standard_normal((m, D)))
    ls, sf2, noise, jitter, jitter_uu = np.array([1.4, 1.6, 1.8]), 1.2, 0.05, 1e-6, 1e-6
    ym, ys = Y.mean(0), Y.std(0)
    tag = f"m={m} D={D} P={P}"
    h = Handle(sparse_panel=256)
    h.sparse_begin(Z, P, ls, sf2, noise, jitter, jitter_uu, ym, ys)
    h.sparse_update(X[:700], Y[:700])
    h.sparse_update(X[700:], Y[700:])
    emit(f"sparse_finalize+bound {tag}", *h.sparse_finalize())
    exported = h.sparse_export(m, D, len(ls))
    emit(f"sparse_export {tag}", *exported)
    for sp in (1, 0):
        h.set(small_path=sp)
        for M in (25, 40):
            for v in (False, True):
                emit(f"sparse_predict {tag} small_path={sp} M={M} var={v}", *h.sparse_predict(Q[:M], v, 1))
    emit(f"sparse_predict {tag} small_path=0 M=40 var=True vin=0", *h.sparse_predict(Q[:40], True, 0))
    h2 = Handle(sparse_panel=256)
    _, Z2, G, g, yy, ls2, hyper, ym2, ys2 = exported
    h2.ok(h2.lib.gpk_sparse_import(h2.h, dp(Z2), m, D, P, dp(ls2), len(ls2), hyper[0], hyper[1], hyper[2], hyper[3], dp(ym2), dp(ys2),
                                   dp(G), dp(g), dp(yy), n))
    h2.P = P
    emit(f"sparse_import+finalize {tag}", *h2.sparse_finalize())
    emit(f"sparse_import+predict {tag} M=25 var=True", *h2.sparse_predict(Q[:25], True, 1))
    h2.close()
    h.close()


def run():
    for N, D, P in ((200, 3, 2), (1000, 10, 6)):
        run_model(N, D, P)
    run_gated()
    for N, D, B in ((301, 10, 6), (130, 16, 8)):
        run_batched(N, D, B)
    for m in (200, 300):
        for P in (1, 3):
            run_sparse(m, P)


def read(f):
    return [line.rsplit(" ", 1) for line in open(f).read().splitlines() if line and not line.startswith("#")]


def compare(files):
    runs = [read(f) for f in files]
    labels = [k for k, _ in runs[0]]
    assert all([k for k, _ in r] == labels for r in runs), "the runs do not print the same lines"
    old, new = (runs[:1], runs[1:]) if len(runs) == 2 else (runs[:2], runs[2:])
    bad = unstable = 0
    for i, k in enumerate(labels):
        d = [r[i][1] for r in runs]
        if any(r[i][1] != old[0][i][1] for r in old):          # the old build does not repeat itself on this line
            unstable += 1
            v = [np.load(os.path.join(f + ".d", f"{i:04d}.npy")) for f in files]
            own = np.abs(v[0] - v[1])
            worst = max(float(np.max(np.abs(n - v[0]) - 2.0 * own)) for n in v[2:])
            state = "UNSTABLE, within twice the old build's own difference" if worst <= 0.0 else "UNSTABLE AND DIFFERENT"
            bad += worst > 0.0
            print(f"{state} {k} (old runs differ by up to {float(own.max()):.3e}; new - old beyond 2x that: {max(worst, 0.0):.3e})")
            continue
        same = all(r[i][1] == d[0] for r in new)
        bad += not same
        print(("equal     " if same else "DIFFERENT ") + k, " ".join(x[:16] for x in d))
    print(f"{len(labels)} lines, {len(old)} run(s) of the old build and {len(new)} of the new: {unstable} unstable between the old "
          f"build's own runs, {bad} different")
    if unstable * 10 > len(labels):
        print("more than one line in ten is unstable: the inputs of this tool are wrong")
        return 1
    return 1 if bad else 0


# ---- timing -----------------------------------------------------------------------------------------------------------------
def cell(label, call, n=1000, warm=200):
    for _ in range(warm):
        call()
    t = np.empty(n)
    for i in range(n):
        t0 = time.perf_counter()
        call()
        t[i] = time.perf_counter() - t0
    p10, med, p90 = np.percentile(t * 1e6, [10, 50, 90])
    print(f"{label} | {med:.1f} {p10:.1f} {p90:.1f}", flush=True)


def run_time():
    _, X, Y, Q = problem(1000, 10, 6, 1000)
    h = Handle()
    h.fit(X, Y, 1.2 + 0.05 * np.arange(10), 1.3, 0.05, 1e-6)
    for M in (1, 25):
        cell(f"gpk_predict f64 var N=1000 P=6 M={M}", lambda: h.predict(Q[:M], True, 1))
    hb = Handle()
    hb.fit_batched(X, Y, np.ascontiguousarray(np.tile(1.2 + 0.05 * np.arange(10), (6, 1)) * (1 + 0.1 * np.arange(6))[:, None]),
                   np.full(6, 1.3), np.full(6, 0.05), 1e-6)
    cell("gpk_predict_batched var B=6 N=1000 M=25", lambda: hb.predict_batched(Q[:25], True, 1))
    cell("gpk_predict_model_grad all four N=1000 P=6 M=25", lambda: h.grad(Q[:25], True, 1))
    cell("gpk_predict_model_cov N=1000 P=6 M=25", lambda: h.cov(Q[:25]))
    cell("gpk_predict_batched_grad all four B=6 N=1000 M=25", lambda: hb.grad_batched(Q[:25], True, 1))
    cell("gpk_predict_batched_cov B=6 N=1000 M=25", lambda: hb.cov_batched(Q[:25]))
    hb.close()
    rng, Xs, Ys, Qs = problem(8192, 3, 1, 5)
    hs = Handle()
    Z = np.ascontiguousarray(Xs[rng.choice(8192, 1024, replace=False)])
    hs.sparse_begin(Z, 1, np.array([1.5]), 1.2, 0.05, 1e-6, 1e-6, Ys.mean(0), Ys.std(0))
    hs.sparse_update(Xs, Ys)
    hs.sparse_finalize()
    for M in (1, 25):
        cell(f"gpk_sparse_predict var m=1024 P=1 M={M}", lambda: hs.sparse_predict(Qs[:M], True, 1))
    cell("gpk_sparse_predict_grad all four m=1024 P=1 M=25", lambda: hs.sparse_grad(Qs[:25], 3))
    cell("gpk_sparse_predict_cov m=1024 P=1 M=25", lambda: hs.sparse_cov(Qs[:25]))
    axes = [hs]
    for b in range(1, 6):      # five more single-output models on the same inducing inputs, each with its own targets and kernel
        ha = Handle()
        ha.sparse_begin(Z, 1, np.array([1.5 + 0.1 * b]), 1.2, 0.05, 1e-6, 1e-6, Ys.mean(0), Ys.std(0))
        ha.sparse_update(Xs, np.ascontiguousarray(np.roll(Ys, 17 * b, axis=0)))
        ha.sparse_finalize()
        axes.append(ha)
    cell("gpk_sparse_predict_multi var B=6 m=1024 M=25", lambda: hs.sparse_predict_multi(axes, Qs[:25]))
    for ha in axes[1:]:
        ha.close()
    hs.close()
    cell(f"gpk_predict f64 var N=1000 P=6 M={BIG}", lambda: h.predict(Q, True, 1), 300, 50)
    h.close()


def time_table(files):
    runs = [dict((k.strip(), [float(x) for x in v.split()]) for k, v in (line.split("|") for line in open(f) if "|" in line))
            for f in files]
    o1, n1, o2, n2 = runs
    rel = max(abs(o1[k][0] - o2[k][0]) / min(o1[k][0], o2[k][0]) for k in o1)
    print(f"Median (10th - 90th percentile) in us per call; runs in the order old, new, old, new in one job.  Largest relative "
          f"old-to-old difference of any cell: {100 * rel:.2f} %.\n")
    print("| cell | old 1 | new 1 | old 2 | new 2 | allowed | verdict |\n|---|---|---|---|---|---|---|")
    failed = 0
    for k in o1:
        a, b = sorted((o1[k][0], o2[k][0]))
        w = max(b - a, rel * a)
        ok = all(a - w <= r[k][0] <= b + w for r in (n1, n2))
        failed += not ok
        cells = " | ".join(f"{r[k][0]:.1f} ({r[k][1]:.1f} - {r[k][2]:.1f})" for r in (o1, n1, o2, n2))
        print(f"| {k} | {cells} | {a - w:.1f} .. {b + w:.1f} | {'pass' if ok else 'FAIL'} |")
    return 1 if failed else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if a[:1] == ["--compare"] and len(a) in (3, 5):
        sys.exit(compare(a[1:]))
    if a[:1] == ["--time-table"] and len(a) == 5:
        sys.exit(time_table(a[1:]))
    if a == ["--time"]:
        run_time()
    else:
        if a[:1] == ["--dump"]:
            _dump_dir = a[1]
            os.makedirs(_dump_dir, exist_ok=True)
        run()
