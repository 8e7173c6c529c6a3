"""The device buffers behind the composite C entries (gpk_dev, csrc/gpk_compose.h) over the life of ONE handle, with the
debug_fill option on (every staging request is overwritten with NaN bytes): staging that grows, grows again and is then
reused with NaN-filled slack, and models that replace one another.  Every result must equal the same call on a fresh
handle bit for bit - an owner that frees too early, too late or twice, or a panel that reads beyond what it wrote, shows
here."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 16384 + 130        # two query panels, the second ragged
SIZES = (300, BIG, 40)   # grown, grown again, reused with slack


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class _Handle:
    def __init__(self):
        from unmanned_aerial_vehicles_amd import _lib
        self._lib, self.lib, self.h = _lib, _lib.load(), C.c_void_p()
        assert self.lib.gpk_create(C.byref(self.h), 0) == _lib.GPK_OK
        self.ok(self.lib.gpk_set_stream(self.h, C.c_void_p(-1)))
        self.ok(self.lib.gpk_set_option(self.h, b"debug_fill", 1))

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
