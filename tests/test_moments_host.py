"""Host-side checks of exact moment matching (DESIGN.md, K11 "moment matching"); no device is touched.

`moments_numpy_form` below is the expected value of every GPU test of `predict_moments` and `propagate(method="moment")`: a dense
NumPy form of the closed-form moments of the posterior at a Gaussian query that builds the N x N matrix L explicitly, from R^-1 S
itself (no Cholesky factor of it, no split exponent: another route than the kernels').

1. Plumbing: the four C entries are declared, bound and exported; the package surface.
2. The form itself against tensor Gauss-Hermite quadrature of the model's own NumPy posterior (`gp_numpy_form.stage`) over the
   state block, on the cases a, b, one (12 nodes per dimension) and csv (nx = 6: 6 nodes) of tests/golden/paths_ref.npz at
   Sigma = 1e-3 V V^T: mean, V and xcov to the quadrature's own error, measured as the difference between two node counts
   and never below cond(K) eps, the rounding of the integrand (asserted against 10 x the larger, both printed); one full stage x_1, Sigma_1 at an SPD Sigma_0 the same way; on a 60-row synthetic model against 16-node quadrature at 1.5e-12.
3. Sigma = 0 reproduces the posterior's mean and variance with xcov = 0; the moment recursion at Sigma0 = 0, H = 1 is the linear
   `host_loop`.
4. What the bar of the GPU tests rests on, printed and asserted: max E[v] above the floor on every case (the clip is inactive),
   and the fp64 form within 1e-10 (of each array's largest entry) of the same form evaluated in np.longdouble from the training
   data on - factorisation, K^-1, weights and sums.
5. The Python-side argument checks (before any device call)."""
import ctypes
import itertools
import os

import numpy as np
import pytest
from scipy.linalg import cho_solve

from conftest import ROOT
from test_propagate_host import axis_form, gp_numpy_form, single_form, spd

NEW_SYMBOLS = ("gpk_moments_host", "gpk_moments_host_multi", "gpk_propagate_mm_host", "gpk_propagate_mm_host_multi")
CASES = {"a": 12, "b": 12, "one": 12, "csv": 6}          # quadrature nodes per state dimension


def _inv(A):
    """Gauss-Jordan inverse and log-determinant of a small SPD matrix in A's own dtype (np.linalg has no longdouble)"""
    n = len(A)
    M = np.concatenate([A.copy(), np.eye(n, dtype=A.dtype)], axis=1)
    logdet = A.dtype.type(0)
    for c in range(n):
        logdet += np.log(M[c, c])
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, n:], logdet


def _chol_inv(K):
    """K^-1 of an SPD matrix through its Cholesky factor, in K's own dtype"""
    n = len(K)
    L = np.zeros_like(K)
    for c in range(n):
        L[c, c] = np.sqrt(K[c, c] - L[c, :c] @ L[c, :c])
        L[c + 1:, c] = (K[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
    W = np.zeros_like(K)                                  # W = L^-1, row by row
    for r in range(n):
        e = np.zeros(n, dtype=K.dtype)
        e[r] = 1
        W[r] = (e - L[r, :r] @ W[:r]) / L[r, r]
    return W.T @ W


class moments_numpy_form:
    """Exact moments of a list of `gp_numpy_form`s (their outputs one after the other) behind in_scaler = (shift, scale) or None
    and out = (mean, scale) per output or None.  dtype np.longdouble: everything from the training data on in extended precision.

    .moments(q (D,) raw, Sraw (nx, nx), noisy) -> mean (NO,), V (NO, NO), xcov (NO, D) in raw units, and E[v] (NO,) unclipped in
    normalised units."""

    def __init__(self, gps, in_scaler=None, out=None, alpha=None, dtype=np.float64):
        self.dt = dt = np.dtype(dtype)
        self.gps, self.in_scaler = gps, in_scaler
        self.NO = sum(len(g.ym) for g in gps)
        self.out = (np.zeros(self.NO), np.ones(self.NO)) if out is None else (np.asarray(out[0], float), np.asarray(out[1], float))
        self.model = []
        for i, g in enumerate(gps):
            X, ls = g.X.astype(dt), g.ls.astype(dt)
            if dt == np.float64:
                Kinv = cho_solve((g.L, True), np.eye(len(X)))
                a = g.alpha
            else:                                         # (alpha[i]: the jitter the float64 form was factored with)
                d = (X / ls)[:, None, :] - (X / ls)[None, :, :]
                K = dt.type(g.sf2) * np.exp(-np.sum(d * d, axis=2) / 2) + (dt.type(g.noise) + dt.type(alpha[i])) * np.eye(len(X), dtype=dt)
                Kinv = _chol_inv(K)
                a = Kinv @ g.Yn.astype(dt)
            self.model.append((X, ls, dt.type(g.sf2), a, Kinv))

    def moments(self, q, Sraw, noisy):
        dt = self.dt
        D = len(q)
        nx = len(Sraw)
        shift, scale = (np.zeros(D), np.ones(D)) if self.in_scaler is None else self.in_scaler
        shift, scale = np.asarray(shift, dt), np.asarray(scale, dt)
        z = (np.asarray(q, dt) - shift) / scale
        S = np.zeros((D, D), dtype=dt)
        S[:nx, :nx] = np.asarray(Sraw, dt) / np.outer(scale[:nx], scale[:nx])
        I = np.eye(D, dtype=dt)
        Emu, Cz, owner = [], [], []
        for g, (X, ls, sf2, a, _) in enumerate(self.model):
            nu = X - z
            Binv, logdet = _inv(S + np.diag(ls ** 2))
            logdet -= np.sum(np.log(ls ** 2))             # log |I + S P|
            l = sf2 * np.exp(-logdet / 2 - np.einsum("nd,de,ne->n", nu, Binv, nu) / 2)
            for p in range(a.shape[1]):
                Emu.append(a[:, p] @ l)
                Cz.append(S @ Binv @ (nu.T @ (a[:, p] * l)))
                owner.append((g, p))
        Emu, Cz = np.array(Emu), np.array(Cz)
        NO = self.NO
        V, Ev = np.zeros((NO, NO), dtype=dt), np.zeros(NO, dtype=dt)
        Ls = {}
        for o, (ga, pa) in enumerate(owner):
            for o2, (gb, pb) in enumerate(owner[:o + 1]):
                if (ga, gb) not in Ls:
                    Xa, lsa, sfa, _, _ = self.model[ga]
                    Xb, lsb, sfb, _, _ = self.model[gb]
                    Pa, Pb = 1 / lsa ** 2, 1 / lsb ** 2
                    Rinv, logR = _inv((S * (Pa + Pb)[None, :] + I).T)       # (the transpose: similar to an SPD matrix, same determinant)
                    Mm = Rinv.T @ S
                    za, zb = (Xa - z) * Pa, (Xb - z) * Pb
                    ea = np.log(sfa) - np.sum(za * (Xa - z), axis=1) / 2 + np.einsum("nd,de,ne->n", za, Mm, za) / 2
                    eb = np.log(sfb) - np.sum(zb * (Xb - z), axis=1) / 2 + np.einsum("nd,de,ne->n", zb, Mm, zb) / 2
                    Ls[(ga, gb)] = np.exp(ea[:, None] + eb[None, :] + za @ Mm @ zb.T - logR / 2)
                L = Ls[(ga, gb)]
                V[o, o2] = V[o2, o] = self.model[ga][3][:, pa] @ L @ self.model[gb][3][:, pb] - Emu[o] * Emu[o2]
            g = self.gps[ga]
            Ev[o] = dt.type(g.sf2 + (g.noise if noisy else 0.0)) - np.sum(self.model[ga][4] * Ls[(ga, ga)])
            V[o, o] += max(Ev[o], dt.type(0))
        ym, ys = np.concatenate([g.ym for g in self.gps]).astype(dt), np.concatenate([g.ys for g in self.gps]).astype(dt)
        om, os_ = self.out[0].astype(dt), self.out[1].astype(dt)
        s = os_ * ys
        return om + os_ * (ym + ys * Emu), V * np.outer(s, s), Cz * s[:, None] * scale[None, :], Ev

    def batch(self, Q, Sraw, noisy):
        """rows Q (M, D) with covariances Sraw (M, nx, nx) -> mean (M, NO), V (M, NO, NO), xcov (M, NO, D) as float64"""
        out = [self.moments(q, s, noisy)[:3] for q, s in zip(Q, Sraw)]
        return tuple(np.array([o[i] for o in out], dtype=np.float64) for i in range(3))

    def run(self, coord, x0, U, lin, Sigma0=None, Q=None, noisy=False):
        """The moment recursion written out here (nothing of the package's): output o drives state coordinate coord[o],
            x_{h+1}[c_o] += mean_o,   Sigma_{h+1} = A0 Sigma_h A0^T + Q, plus, per pair of outputs (o, p),
            V_op at [c_o][c_p], and per output o the column A0 Cov[x, y_o] at [:, c_o] with its transpose at [c_o, :].
        x0 (R, nx), U (R, H, nu) -> traj (H + 1, R, nx), Sigma (H + 1, R, nx, nx), {"mean", "cov", "xcov"}."""
        coord = [int(c) for c in coord]
        nx, D = lin.shape
        R, H, NO = U.shape[0], U.shape[1], self.NO
        traj, Sigma = np.zeros((H + 1, R, nx)), np.zeros((H + 1, R, nx, nx))
        st = {"mean": np.zeros((H, R, NO)), "cov": np.zeros((H, R, NO, NO)), "xcov": np.zeros((H, R, NO, D))}
        traj[0] = x0
        if Sigma0 is not None:
            Sigma[0] = Sigma0
        A0 = np.eye(nx) + lin[:, :nx]
        for h in range(H):
            for r in range(R):
                q = np.concatenate([traj[h, r], U[r, h]])
                mean, V, xcov = (np.asarray(a, dtype=np.float64) for a in self.moments(q, Sigma[h, r], noisy)[:3])
                x = traj[h, r] + lin @ q
                S = A0 @ Sigma[h, r] @ A0.T + (0.0 if Q is None else Q)
                for o, c in enumerate(coord):
                    x[c] += mean[o]
                    col = A0 @ xcov[o, :nx]
                    S[:, c] += col
                    S[c, :] += col
                    for p, c2 in enumerate(coord):
                        S[c, c2] += V[o, p]
                traj[h + 1, r], Sigma[h + 1, r] = x, S
                st["mean"][h, r], st["cov"][h, r], st["xcov"][h, r] = mean, V, xcov
        return traj, Sigma, st


def form_of(name, dtype=np.float64):
    """(the fixture's arrays, the propagate form, the moments form) of a single-model case of paths_ref.npz"""
    c, pform = single_form(name)
    g = pform.gps[0]
    if not hasattr(g, "Yn"):
        Y = c["Y"].reshape(len(c["X"]), -1)
        g.Yn = (Y - g.ym) / g.ys
    return c, pform, moments_numpy_form(pform.gps, alpha=[c["hyper"][2]], dtype=dtype)


def gaussian_query(c, scale=1e-3, seed=11):
    """a query row of the fixture (its first start and control) and Sigma = scale V V^T on the state block"""
    nx = c["lin"].shape[0]
    V = np.random.default_rng(seed).standard_normal((nx, nx))
    S = scale * (V @ V.T)
    return np.concatenate([c["x0"][0], c["U"][0]]), 0.5 * (S + S.T)


_quadratures = {}


def case_quadrature(name, nodes):
    """`gauss_hermite` of a fixture case at its `gaussian_query`: computed once per (case, node count), shared, left unchanged"""
    if (name, nodes) not in _quadratures:
        c, pform, _ = form_of(name)
        _quadratures[(name, nodes)] = gauss_hermite(pform, *gaussian_query(c), nodes)
    return _quadratures[(name, nodes)]


def gauss_hermite(pform, q, S, nodes, noisy=False, chunk=4096):
    """E[mu], Cov[mu] + diag E[v], Cov[q, mu] of the form's own posterior under q_x ~ N(q[:nx], S) by tensor Gauss-Hermite"""
    nx = len(S)
    x, w = np.polynomial.hermite.hermgauss(nodes)
    C = np.linalg.cholesky(S)
    grid = np.array(list(itertools.product(range(nodes), repeat=nx)))
    W = np.prod(w[grid], axis=1) / np.pi ** (nx / 2)
    dev = np.sqrt(2.0) * x[grid] @ C.T
    m1 = m2 = mv = mx = 0.0
    for s in range(0, len(grid), chunk):
        Q = np.tile(q, (len(dev[s:s + chunk]), 1))
        Q[:, :nx] += dev[s:s + chunk]
        mean, _, var = pform.stage(Q, noisy)
        ww = W[s:s + chunk]
        m1 = m1 + ww @ mean
        m2 = m2 + np.einsum("n,np,nq->pq", ww, mean, mean)
        mv = mv + ww @ var
        mx = mx + np.einsum("n,np,nd->pd", ww, mean, dev[s:s + chunk])
    xcov = np.zeros((len(m1), len(q)))
    xcov[:, :nx] = mx
    return m1, m2 - np.outer(m1, m1) + np.diag(mv), xcov


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, float) - np.asarray(b, float))) / max(np.max(np.abs(b)), 1e-300))


# ---- 1. plumbing -------------------------------------------------------------------------------------------------------------------
def test_libgpk_exports_the_moment_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES
    assert "gpk_moments.hip" in _build.SOURCES
    assert len(_lib.SIGNATURES["gpk_propagate_mm_host"][1]) == len(_lib.SIGNATURES["gpk_propagate_host"][1])
    assert len(_lib.SIGNATURES["gpk_moments_host"][1]) == 24 and len(_lib.SIGNATURES["gpk_moments_host_multi"][1]) == 26


def test_package_surface():
    import inspect
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd.device import DeviceGP
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    from unmanned_aerial_vehicles_amd.sparse_batch import BatchedSparseGP
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    for cls in (pkg.GaussianProcessRegressor, pkg.BatchedARDGP):
        assert callable(getattr(cls, "predict_moments", None)), cls
    for fn in (pkg.GaussianProcessRegressor.propagate, pkg.BatchedARDGP.propagate, SparseGP.propagate, BatchedSparseGP.propagate,
               pkg.GaussianProcessRegressor.propagate_gradient, pkg.BatchedARDGP.propagate_gradient,
               pkg.SimpleQuadrotorGP.propagate_horizon, PreTrainedGP.propagate_horizon):
        assert inspect.signature(fn).parameters["method"].default == "linear", fn
    assert callable(DeviceGP.moments_ok) and callable(DeviceGP.inverse_gram)


# ---- 2. the form against quadrature ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_form_matches_gauss_hermite(name):
    c, pform, mform = form_of(name)
    q, S = gaussian_query(c)
    n = CASES[name]
    fine, coarse = case_quadrature(name, n), case_quadrature(name, n - 2 if n > 6 else n - 1)
    got = mform.moments(q, S, False)[:3]
    cond = np.linalg.cond(pform.gps[0].L) ** 2
    for tag, g, f, k in zip(("mean", "V", "xcov"), got, fine, coarse):
        # the quadrature's own error: two node counts against each other, and the rounding of its integrand - every node's
        # variance is kss - k*^T K^-1 k* through a float64 factorisation, relative error cond(K) eps
        nodes, floor = rel(k, f), cond * np.finfo(float).eps
        own = max(nodes, floor)
        err = rel(g, f)
        print(f"{name} {tag}: form against {n}-node quadrature {err:.2e}; quadrature's own error: two node counts {nodes:.2e}, "
              f"rounding of its integrand cond(K) eps {floor:.2e}; asserted against 10 x {own:.2e}")
        assert err <= 10 * own, (name, tag, err, own)


def stage_from(q, S, lin, Q, moments):
    """x_1 and Sigma_1 of one stage from the moments (mean, V, xcov) of the outputs, which drive coordinates 0 .. nx - 1"""
    nx = lin.shape[0]
    mean, V, xcov = moments
    A0 = np.eye(nx) + lin[:, :nx]
    F = A0 @ xcov[:, :nx].T
    return q[:nx] + lin @ q + mean, A0 @ S @ A0.T + F + F.T + V + Q


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_full_stage_matches_gauss_hermite(name):
    """x_1 and Sigma_1 of the form's recursion at an SPD Sigma_0 and a process noise against the stage composed from quadrature
    moments: the cross terms A0 Cx E^T + E Cx^T A0^T and E V E^T against other code than the kernels' and the package's"""
    c, pform, mform = form_of(name)
    q, S = gaussian_query(c)
    n = CASES[name]
    nx = c["lin"].shape[0]
    _, Q = spd(nx)
    fine = stage_from(q, S, c["lin"], Q, case_quadrature(name, n))
    coarse = stage_from(q, S, c["lin"], Q, case_quadrature(name, n - 2 if n > 6 else n - 1))
    traj, Sigma, _ = mform.run(range(nx), q[None, :nx], q[None, None, nx:], c["lin"], S[None], Q)
    cond = np.linalg.cond(pform.gps[0].L) ** 2
    for tag, g, f, k in (("x_1", traj[1, 0], fine[0], coarse[0]), ("Sigma_1", Sigma[1, 0], fine[1], coarse[1])):
        nodes, floor = rel(k, f), cond * np.finfo(float).eps
        err = rel(g, f)
        print(f"{name} {tag}: form against {n}-node quadrature {err:.2e}; two node counts {nodes:.2e}, cond(K) eps {floor:.2e}")
        assert err <= 10 * max(nodes, floor), (name, tag, err)


def test_host_loop_moments_is_the_forms_recursion():
    """the package's host recursion (`route="host"`) on the form's moments against the recursion written in the form, on a batch
    with a coordinate map that leaves coordinates free, an SPD Sigma_0 and a process noise"""
    from unmanned_aerial_vehicles_amd.propagate import host_loop_moments
    c, pform = axis_form("gap")
    mform = moments_numpy_form(pform.gps, pform.in_scaler, pform.out)
    nx = c["lin"].shape[0]
    S0, Q = spd(nx)
    x0, U = c["x0"][:1] + 0.01 * np.arange(2)[:, None], np.tile(c["U"][None, :3], (2, 1, 1))
    want = mform.run(pform.coord, x0, U, c["lin"], np.tile(0.05 * S0, (2, 1, 1)), Q)
    got = host_loop_moments(lambda q, S: mform.batch(q, S, False), list(pform.coord), x0, U, c["lin"], 0.05 * S0[None], Q, 2, 3)
    assert rel(got[0], want[0]) <= 1e-13 and rel(got[1], want[1]) <= 1e-13
    assert all(rel(got[2][k], want[2][k]) <= 1e-13 for k in ("mean", "cov", "xcov"))


def synthetic(noise, N=60, seed=5):
    """60 rows spread over twice the unit normal in 3 inputs (length-scales 1.3 .. 2.1: neighbouring rows are not near-duplicates,
    cond(K) stays below 5e4 down to noise 1e-4), two outputs"""
    rng = np.random.default_rng(seed)
    X = 2.0 * rng.standard_normal((N, 3))
    Y = np.stack([np.sin(X[:, 0]) + 0.3 * X[:, 1], np.cos(X[:, 1] - X[:, 2])], axis=1) + np.sqrt(noise) * rng.standard_normal((N, 2))
    g = gp_numpy_form(X, Y, np.array([1.3, 1.7, 2.1]), 1.2, noise, 1e-10)
    g.Yn = (Y - g.ym) / g.ys
    return g


def test_form_matches_16_node_quadrature_on_a_synthetic_model():
    from test_propagate_host import propagate_numpy_form
    # (both sides go through a float64 factorisation of K, relative error cond(K) eps with cond(K) <= 1 + N sf2 / noise: noise
    # 0.1 keeps that below the 1.5e-12 asked of the closed form)
    g = synthetic(1e-1)
    q = np.array([0.2, -0.3, 0.4])
    S = np.array([[0.04, 0.01], [0.01, 0.03]])
    want = gauss_hermite(propagate_numpy_form([g]), q, S, 16)
    got = moments_numpy_form([g]).moments(q, S, False)[:3]
    for tag, a, b in zip(("mean", "V", "xcov"), got, want):
        print(f"synthetic {tag}: {rel(a, b):.2e}")
        assert rel(a, b) <= 1.5e-12, tag


# ---- 3. Sigma = 0 and the linear recursion -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", (False, True))
@pytest.mark.parametrize("name", sorted(CASES))
def test_zero_covariance_is_the_posterior(name, noisy):
    c, pform, mform = form_of(name)
    q, S = gaussian_query(c)
    mean, V, xcov, _ = mform.moments(q, 0.0 * S, noisy)
    pm, _, pv = pform.stage(q[None, :], noisy)
    assert rel(mean, pm[0]) <= 1e-12
    assert rel(np.diag(V), pv[0]) <= 1e-9                 # (two routes to kss - k*^T K^-1 k*: the cancellation of the variance)
    assert np.max(np.abs(V - np.diag(np.diag(V)))) <= 1e-12 * np.max(np.abs(mean)) ** 2 + 1e-18
    assert not xcov.any()


@pytest.mark.parametrize("name", ("b", "csv"))
def test_moment_recursion_at_zero_covariance_is_the_linear_host_loop(name):
    from unmanned_aerial_vehicles_amd.propagate import host_loop, host_loop_moments
    c, pform, mform = form_of(name)
    nx = c["lin"].shape[0]
    x0, U = c["x0"][:3], np.tile(c["U"][None, :1], (3, 1, 1))
    _, Q = spd(nx)
    traj, Sigma, _ = host_loop_moments(lambda q, S: mform.batch(q, S, False), list(range(nx)), x0, U, c["lin"], None, Q, 3, 1)
    t2, S2, _ = host_loop(lambda q: pform.stage(q, False), list(range(nx)), x0, U, c["lin"], None, Q, 3, 1)
    assert rel(traj, t2) <= 1e-12 and rel(Sigma, S2) <= 1e-9


# ---- 4. conditioning: what the GPU bar rests on -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_conditioning_of_the_fixture_cases(name):
    c, _, mform = form_of(name)
    _, _, lform = form_of(name, np.longdouble)
    q, S = gaussian_query(c)
    got, ext = mform.moments(q, S, False), lform.moments(q, S, False)
    floor = 0.0
    print(f"{name}: min E[v] / sf2 = {float(np.min(got[3])) / c['hyper'][0]:.3e} (floor {floor})")
    assert np.min(got[3]) > floor and np.min(got[3]) > 1e-6 * c["hyper"][0]
    for tag, a, b in zip(("mean", "V", "xcov"), got[:3], ext[:3]):
        print(f"{name} {tag}: float64 against longdouble {rel(a, b):.2e}")
        assert rel(a, b) <= 1e-10, tag


@pytest.mark.parametrize("noise", (1e-2, 1e-3, 1e-4))
def test_conditioning_on_synthetic_models(noise):
    """float64 against longdouble (from the training data on) on the 60-row synthetic model, relative to each array's largest
    entry; measured: V 1.1e-12, 6.2e-12, 7.9e-12 at noise 1e-2, 1e-3, 1e-4, mean and xcov <= 1.3e-14"""
    g = synthetic(noise)
    q, S = np.array([0.2, -0.3, 0.4]), np.array([[0.04, 0.01], [0.01, 0.03]])
    got = moments_numpy_form([g]).moments(q, S, False)
    ext = moments_numpy_form([g], alpha=[1e-10], dtype=np.longdouble).moments(q, S, False)
    for tag, a, b in zip(("mean", "V", "xcov"), got[:3], ext[:3]):
        print(f"noise {noise:g} {tag}: float64 against longdouble {rel(a, b):.2e}")
        assert rel(a, b) <= 1e-10, tag


def test_axis_form_pairs_are_consistent():
    """the batch form (six models, scalers): V is PSD up to rounding and its diagonal is the one-model form's"""
    c, pform = axis_form("csv")
    mform = moments_numpy_form(pform.gps, pform.in_scaler, pform.out)
    q = np.concatenate([c["x0"][0], c["U"][0]])
    _, S = gaussian_query({"lin": c["lin"], "x0": c["x0"], "U": c["U"]})
    mean, V, xcov, _ = mform.moments(q, S, False)
    assert np.min(np.linalg.eigvalsh(V)) > -1e-12 * np.max(np.abs(V))
    one = moments_numpy_form(pform.gps[:1], pform.in_scaler, (pform.out[0][:1], pform.out[1][:1])).moments(q, S, False)
    assert rel(one[0], mean[:1]) <= 1e-13 and rel(one[1], V[:1, :1]) <= 1e-12 and rel(one[2], xcov[:1]) <= 1e-12


# ---- 5. argument checks, before any device call -------------------------------------------------------------------------------------
def test_method_checks():
    from unmanned_aerial_vehicles_amd import propagate as pg
    assert pg.check_method("linear", 2) == "linear" and pg.check_method("moment", 1) == "moment"
    with pytest.raises(ValueError, match="order=1"):
        pg.check_method("moment", 2)
    with pytest.raises(ValueError, match="method must be"):
        pg.check_method("exact", 1)
    pg.refuse_moment("linear", "SparseGP")
    with pytest.raises(ValueError, match="SparseGP"):
        pg.refuse_moment("moment", "SparseGP")


def test_indefinite_covariances_are_refused():
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd import propagate as pg
    bad = np.array([[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(ValueError, match="positive semi-definite"):
        pg.check_gaussian_queries(np.zeros((1, 3)), bad, 3)
    with pytest.raises(ValueError, match="Sigma0 must be positive semi-definite"):
        pg.check_method("moment", 1, Sigma0=bad[None])
    pg.check_method("linear", 1, Sigma0=bad[None])
    pg.check_psd(np.zeros((2, 2, 2)), "Sigma")
    pg.check_psd(np.array([[1.0, 1.0], [1.0, 1.0]]), "Sigma")      # singular is fine
    assert callable(pkg.GaussianProcessRegressor.predict_moments)


def test_gaussian_query_checks():
    from unmanned_aerial_vehicles_amd.propagate import check_gaussian_queries
    X, S, M, nx = check_gaussian_queries(np.zeros((3, 4)), np.eye(2), 4)
    assert X.shape == (3, 4) and S.shape == (3, 2, 2) and (M, nx) == (3, 2)
    assert check_gaussian_queries(np.zeros(4), None, 4)[1].shape == (1, 4, 4)
    for bad_X, bad_S in ((np.zeros((3, 5)), np.eye(2)), (np.zeros((33, 4)), np.eye(2)), (np.zeros((3, 4)), np.eye(5)),
                         (np.zeros((3, 4)), np.zeros((2, 2, 2))), (np.zeros((3, 4)), np.array([[1.0, 0.5], [0.0, 1.0]])),
                         (np.full((3, 4), np.nan), np.eye(2)), (np.zeros((3, 4)), np.full((2, 2), np.inf))):
        with pytest.raises(ValueError):
            check_gaussian_queries(bad_X, bad_S, 4)


def test_estimators_refuse_before_any_device_call():
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    gp = pkg.GaussianProcessRegressor()
    with pytest.raises(ValueError, match="order=1"):
        gp.propagate(np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), method="moment", order=2)
    with pytest.raises(ValueError, match="method must be"):
        gp.propagate(np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), method="unscented")
    with pytest.raises(RuntimeError, match="not fitted"):
        gp.predict_moments(np.zeros((1, 3)), np.eye(2))
    with pytest.raises(ValueError, match="propagate_gradient"):
        gp.propagate_gradient(np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), np.zeros((4, 1, 2)), method="moment")
    with pytest.raises(ValueError, match="SparseGP"):
        SparseGP.propagate(SparseGP.__new__(SparseGP), np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), method="moment")
    with pytest.raises(ValueError, match="order=1"):
        pkg.BatchedARDGP(optimizer=None).propagate(np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), method="moment", order=2)


def test_wrappers_fall_back_without_a_model(capsys):
    import unmanned_aerial_vehicles_amd as pkg
    X, Sigma = pkg.SimpleQuadrotorGP().propagate_horizon(np.zeros(6), np.zeros((4, 3)), 0.05, method="moment")
    assert X.shape == (6, 4) and Sigma.shape == (4, 6, 6) and not Sigma.any()
    assert "not trained" in capsys.readouterr().out
    with pytest.raises(ValueError, match="order=1"):
        pkg.SimpleQuadrotorGP().propagate_horizon(np.zeros(6), np.zeros((4, 3)), 0.05, method="moment", order=2)
