"""The device buffers behind the composite C entries (gpk_dev, csrc/gpk_compose.h) over the life of ONE handle, with the
debug_fill option on (every staging request is overwritten with NaN bytes): staging that grows, grows again and is then
reused with NaN-filled slack, models that replace one another, and the work area of the small-batch launches.  Every
result must equal the same call on a fresh handle bit for bit - an owner that frees too early, too late or twice, or a
panel or kernel that reads beyond what was written, shows here."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 16384 + 130        # two query panels, the second ragged
SIZES = (300, BIG, 40)   # grown, grown again, reused with slack


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class _Handle:
    def __init__(self, debug_fill=1):
        from unmanned_aerial_vehicles_amd import _lib
        self._lib, self.lib, self.h = _lib, _lib.load(), C.c_void_p()
        assert self.lib.gpk_create(C.byref(self.h), 0) == _lib.GPK_OK
        self.ok(self.lib.gpk_set_stream(self.h, C.c_void_p(-1)))
        self.ok(self.lib.gpk_set_option(self.h, b"debug_fill", debug_fill))

    def ok(self, rc):
        assert rc == self._lib.GPK_OK, self.lib.gpk_last_error(self.h).decode()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.gpk_destroy(self.h)

    def fit(self, X, Y):
        ls = np.array([1.5])
        self.P = Y.shape[1]
        self.ok(self.lib.gpk_fit(self.h, _dp(X), X.shape[0], X.shape[1], _dp(Y), self.P, _dp(ls), 1, 1.2, 0.05, 1e-6, 1))

    def predict_rc(self, Q):
        mean, var = np.full((len(Q), self.P), -1.0), np.full((len(Q), self.P), -1.0)
        rc = self.lib.gpk_predict(self.h, Q.ctypes.data_as(C.c_void_p), len(Q), mean.ctypes.data_as(C.c_void_p),
                                  var.ctypes.data_as(C.c_void_p), self._lib.GPK_F64, 1)
        return rc, mean, var

    def predict(self, Q):
        rc, mean, var = self.predict_rc(Q)
        self.ok(rc)
        return mean, var

    def fit_batched(self, X, Y):
        B, D = Y.shape[1], X.shape[1]
        ls = np.ascontiguousarray(1.5 + 0.1 * np.arange(B * D).reshape(B, D))
        self.B, info = B, (C.c_int * B)()
        self.ok(self.lib.gpk_fit_batched(self.h, B, _dp(X), X.shape[0], D, _dp(Y), _dp(ls), D, _dp(np.full(B, 1.2)),
                                         _dp(np.full(B, 0.05)), 1e-6, 1, info))

    def predict_batched_rc(self, Q):
        mean, var = np.full((len(Q), self.B), -1.0), np.full((len(Q), self.B), -1.0)
        return self.lib.gpk_predict_batched(self.h, _dp(Q), len(Q), _dp(mean), _dp(var), 1), mean, var

    def predict_batched(self, Q):
        rc, mean, var = self.predict_batched_rc(Q)
        self.ok(rc)
        return mean, var

    def fit_sparse(self, X, Y):
        Z = np.ascontiguousarray(X[::4])
        self.ok(self.lib.gpk_sparse_begin(self.h, _dp(Z), len(Z), Z.shape[1], 1, _dp(np.array([1.5])), 1, 1.2, 0.05, 1e-6, 1e-6,
                                          _dp(np.zeros(1)), _dp(np.ones(1))))
        self.ok(self.lib.gpk_sparse_update(self.h, _dp(X), _dp(np.ascontiguousarray(Y[:, :1])), len(X)))
        info = C.c_int()
        self.ok(self.lib.gpk_sparse_finalize(self.h, C.byref(info)))

    def sparse_predict_rc(self, Q):
        mean, var = np.empty((len(Q), 1)), np.empty((len(Q), 1))
        return self.lib.gpk_sparse_predict(self.h, _dp(Q), len(Q), _dp(mean), _dp(var), 1), mean, var

    def fit_sparse_outputs(self, X, Y, m):
        """m inducing inputs, every column of Y an output with a normalisation of its own."""
        Z, self.P = np.ascontiguousarray(X[:m]), Y.shape[1]
        ls = np.ascontiguousarray(1.5 + 0.1 * np.arange(X.shape[1]))
        self.ok(self.lib.gpk_sparse_begin(self.h, _dp(Z), m, Z.shape[1], self.P, _dp(ls), len(ls), 1.2, 0.05, 1e-6, 1e-6,
                                          _dp(np.ascontiguousarray(Y.mean(0))), _dp(np.ascontiguousarray(1.0 + 0.5 * np.arange(self.P)))))
        self.ok(self.lib.gpk_sparse_update(self.h, _dp(X), _dp(Y), len(X)))
        info = C.c_int()
        self.ok(self.lib.gpk_sparse_finalize(self.h, C.byref(info)))

    def small_calls(self, sparse, Q):
        """Every call the small-batch launches serve, on the exact model (gpk_fit) or the sparse one: mean, mean + variance,
        mean + Jacobian, all four gradient results, mean + covariance.  The outputs start as NaN."""
        lib, M, P, D = self.lib, len(Q), self.P, Q.shape[1]

        def nan(*shape):
            return np.full(shape, np.nan)

        results = []
        for want_var in (False, True):
            mean, var = nan(M, P), nan(M, P) if want_var else None
            if sparse:
                self.ok(lib.gpk_sparse_predict(self.h, _dp(Q), M, _dp(mean), _dp(var), 1))
            else:
                self.ok(lib.gpk_predict(self.h, Q.ctypes.data_as(C.c_void_p), M, mean.ctypes.data_as(C.c_void_p),
                                        None if var is None else var.ctypes.data_as(C.c_void_p), self._lib.GPK_F64, 1))
            results.append((mean, var))
            mean, dmean = nan(M, P), nan(M, P, D)
            var, dvar = (nan(M, P), nan(M, P, D)) if want_var else (None, None)
            grad = lib.gpk_sparse_predict_grad if sparse else lib.gpk_predict_model_grad
            self.ok(grad(self.h, _dp(Q), M, _dp(mean), _dp(var), _dp(dmean), _dp(dvar), 1))
            results.append((mean, var, dmean, dvar))
        mean, cov = nan(M, P), nan(P, M, M)
        self.ok((lib.gpk_sparse_predict_cov if sparse else lib.gpk_predict_model_cov)(self.h, _dp(Q), M, _dp(mean), _dp(cov)))
        results.append((mean, cov))
        return [a for r in results for a in r if a is not None]


def _problem(N, D, P):
    rng = np.random.default_rng(N + P)
    X = rng.standard_normal((N, D))
    Y = np.ascontiguousarray(np.sin(X @ rng.standard_normal((D, P))) + 0.1 * rng.standard_normal((N, P)))
    return X, Y, np.ascontiguousarray(1.1 * rng.standard_normal((BIG, D)))


def _same_as_fresh_handles(fit, predict, X, Y, Q):
    with _Handle() as h:
        getattr(h, fit)(X, Y)
        got = [getattr(h, predict)(Q[:M]) for M in SIZES]
    for M, (mean, var) in zip(SIZES, got):
        with _Handle() as fresh:
            getattr(fresh, fit)(X, Y)
            want_mean, want_var = getattr(fresh, predict)(Q[:M])
        assert np.isfinite(mean).all() and np.isfinite(var).all(), M
        assert np.array_equal(mean, want_mean) and np.array_equal(var, want_var), M


def test_predict_staging_grown_regrown_and_reused():
    """(a) gpk_fit at N = 200, then gpk_predict at M = 300, 16 384 + 130 and 40 on the one handle."""
    _same_as_fresh_handles("fit", "predict", *_problem(200, 3, 2))


def test_predict_batched_staging_grown_regrown_and_reused():
    """(b) the same three sizes through gpk_predict_batched with B = 2 and N = 130."""
    _same_as_fresh_handles("fit_batched", "predict_batched", *_problem(130, 3, 2))


def test_models_replaced_and_released():
    """(c) gpk_fit on a handle that already holds a model, a batched model and a sparse model, then gpk_model_release: each of
    the three predict entries refuses with GPK_BAD_ARG, and a new gpk_fit + gpk_predict at M = 33 equals a fresh handle's."""
    X, Y, Q = _problem(200, 3, 2)
    X2, Y2, _ = _problem(130, 3, 2)
    with _Handle() as h:
        h.fit(X2, Y2)
        h.predict(Q[:300])                      # staging and the inverse factor of the model that is replaced below
        h.fit_batched(X2, Y2)
        h.predict_batched(Q[:300])
        h.fit_sparse(X, Y)
        assert h.sparse_predict_rc(Q[:40])[0] == h._lib.GPK_OK
        h.fit(X, Y)
        h.predict(Q[:300])
        h.ok(h.lib.gpk_model_release(h.h))
        bad = h._lib.GPK_BAD_ARG
        assert h.predict_rc(Q[:33])[0] == bad and h.predict_batched_rc(Q[:33])[0] == bad and h.sparse_predict_rc(Q[:33])[0] == bad
        h.fit(X, Y)
        mean, var = h.predict(Q[:33])
    with _Handle() as fresh:
        fresh.fit(X, Y)
        want_mean, want_var = fresh.predict(Q[:33])
    assert np.isfinite(var).all() and np.array_equal(mean, want_mean) and np.array_equal(var, want_var)


@pytest.mark.parametrize("sparse", (False, True), ids=("exact", "sparse"))
def test_small_batch_work_area_is_written_before_it_is_read(sparse):
    """(d) every small-batch call - predict and gradients without and with variances, covariance - at M = 16 and 17 (the
    two tile forms) on one handle with debug_fill on: the exact model (one inverse factor, N = 200, D = 3, P = 2) and the
    sparse one (two, m = 130, D = 4, P = 3), both at the smallest padded size, 256.  One launch routine hands every kernel
    its part of the work area; a kernel that reads what nobody wrote reads NaN.  Every output is finite and has the bits of
    the same call on a fresh handle with debug_fill off."""
    X, Y, Q = _problem(200, 4, 3) if sparse else _problem(200, 3, 2)
    fit = (lambda h: h.fit_sparse_outputs(X, Y, 130)) if sparse else (lambda h: h.fit(X, Y))
    with _Handle() as h:
        fit(h)
        got = {M: h.small_calls(sparse, Q[:M]) for M in (16, 17)}
    for M, arrays in got.items():
        with _Handle(debug_fill=0) as fresh:
            fit(fresh)
            want = fresh.small_calls(sparse, Q[:M])
        assert len(arrays) == len(want) == 11
        for i, (a, w) in enumerate(zip(arrays, want)):
            assert np.isfinite(a).all(), (M, i)
            assert np.array_equal(a, w), (M, i)
