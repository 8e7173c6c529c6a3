"""Host-side checks of the second-order horizon propagation (DESIGN.md, K11 "second order"); no device is touched.

`propagate2_numpy_form` below is the expected value of the GPU tests of `order=2`: `propagate_numpy_form`'s recursion with

    c_b     = 1/2 sum_{d,e < nx} H_b[d][e] Sigma_h[d][e]        H_b = d2 mu_b / dq2 in raw units at q = [x_h, u_h]
    x_{h+1} = (x_h + lin q + sum_b e_coord[b] mu_b) + sum_b e_coord[b] c_b

and A_h, Sigma_{h+1} unchanged.  The Hessian is the closed form of tests/golden/make_golden_hess.py, checked here against
tests/golden/hess_ref.npz before anything rests on it.

1. Plumbing: the four C entries are declared, bound and exported; `order` is on the six Python surfaces; order=3 is a ValueError.
2. The order of the error: for x ~ N(x0, s V V^T) (V the Q factor of default_rng(0).standard_normal((nx, 2)); one column at
   nx = 1) the exact E[x_1] by
   14-node Gauss-Hermite quadrature of the first-order form's step.  The first-order prediction errs by O(s), the corrected one
   by O(s^2): at s = 6.25e-3 and s / 4 the corrected error is the smaller, falls by >= 8x (a fourth-order remainder gives 16;
   measured 15.7 .. 16.0) while the first-order error falls by <= 6x (measured 3.8 .. 4.0).
3. With Sigma0 = 0 and Q = 0 the first stage has nothing to correct.
4. The control-loop wrappers without a model, at order 2."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, relerr
from test_propagate_host import SINGLE_CASES, _nominal_sigma, gp_numpy_form, propagate_numpy_form, rbf, single_form, spd

NEW_SYMBOLS = ("gpk_propagate2_host", "gpk_propagate2_host_multi", "gpk_sparse_propagate2", "gpk_sparse_propagate2_multi")


def mean_model(g):
    """(inputs (N, D), alpha (N, P), ls (D,), sf2, y_std (P,)) of the exact form behind a stage model's MEAN: a `gp_numpy_form`'s own
    arrays, or (Z, alpha_u) of a `sparse_numpy_form` (alpha_u as tests/test_gpu_sparse_batch.py: numpy_form forms it)."""
    if hasattr(g, "alpha"):
        return g.X, g.alpha, g.ls, g.sf2, g.ys
    from scipy.linalg import cho_solve, cholesky
    if hasattr(g, "p"):         # sparse_numpy_form: one output
        p = g.p
        X, Yn, Z, ls, sf2, s2 = p["X"], ((p["y"] - p["ym"]) / p["ys"])[:, None], p["Z"], p["ls"], p["sf2"], p["noise"] + g.a
    else:                       # dense_sparse_form (tests/test_sparse_propagate_host.py): P outputs on one kernel
        X, Y, Z, ls, sf2, noise, alpha = g.a
        Yn, s2 = (Y - g.ym) / g.ys, noise + alpha
    ls = np.broadcast_to(np.asarray(ls, dtype=float), (X.shape[1],))
    Kuu = rbf(Z, Z, ls, sf2) + 1e-8 * sf2 * np.eye(len(Z))
    Kuf = rbf(Z, X, ls, sf2)
    au = cho_solve((cholesky(Kuu + Kuf @ Kuf.T / s2, lower=True), True), Kuf @ Yn) / s2
    return Z, au, ls, sf2, np.reshape(g.ys, (-1,))


def closed_form_hessian(X, alpha, ls, sf2, ystd, Zq):
    """tests/golden/make_golden_hess.py: hess[m][p][d][e] = y_std[p] / (ls_d ls_e) sum_j k_j alpha_jp (delta_jd delta_je - [d = e])
    with delta_j = (z - x_j) / ls; (M, P, D, D)."""
    D = X.shape[1]
    ls = np.broadcast_to(np.asarray(ls, dtype=float), (D,))
    delta = (Zq / ls)[:, None, :] - (X / ls)[None, :, :]
    w = (sf2 * np.exp(-0.5 * np.sum(delta * delta, axis=2)))[:, :, None] * alpha[None, :, :]      # (M, N, P)
    T = np.einsum("mnp,mnd,mne->mpde", w, delta, delta) - np.sum(w, axis=1)[:, :, None, None] * np.eye(D)
    return np.reshape(ystd, (1, -1, 1, 1)) / (ls[:, None] * ls[None, :]) * T


class propagate2_numpy_form(propagate_numpy_form):
    """`propagate_numpy_form` at second order.  .hess(q) -> (R, NO, D, D) in RAW units behind the scalers;
    .run2(...) -> traj, Sigma, the stages of `run` plus "corr" (H, R, NO)."""

    def hess(self, q):
        D = q.shape[1]
        shift, scale = (np.zeros(D), np.ones(D)) if self.in_scaler is None else self.in_scaler
        Hs = np.concatenate([closed_form_hessian(*mean_model(g), (q - shift) / scale) for g in self.gps], axis=1)
        return self.out[1][None, :, None, None] * Hs / (scale[:, None] * scale[None, :])

    def corr(self, q, Sigma):
        nx = Sigma.shape[-1]
        return 0.5 * np.einsum("rode,rde->ro", self.hess(q)[:, :, :nx, :nx], Sigma)

    def run2(self, x0, U, lin, Sigma0=None, Q=None, noisy=False):
        nx, D = lin.shape
        R, H = U.shape[0], U.shape[1]
        traj, Sigma = np.zeros((H + 1, R, nx)), np.zeros((H + 1, R, nx, nx))
        st = {"mean": np.zeros((H, R, self.NO)), "var": np.zeros((H, R, self.NO)), "jac": np.zeros((H, R, self.NO, D)),
              "corr": np.zeros((H, R, self.NO))}
        traj[0] = x0
        if Sigma0 is not None:
            Sigma[0] = Sigma0
        for h in range(H):
            nxt, mean, jac, var = self.step(traj[h], U[:, h], lin, noisy)
            c = self.corr(np.concatenate([traj[h], U[:, h]], axis=1), Sigma[h])
            nxt[:, self.coord] += c
            A = np.tile(np.eye(nx) + lin[:, :nx], (R, 1, 1))
            A[:, self.coord, :] += jac[:, :, :nx]
            S = A @ Sigma[h] @ A.transpose(0, 2, 1)
            S[:, self.coord, self.coord] += var
            if Q is not None:
                S = S + Q
            traj[h + 1], Sigma[h + 1] = nxt, S
            st["mean"][h], st["var"][h], st["jac"][h], st["corr"][h] = mean, var, jac, c
        return traj, Sigma, st


def second(form):
    """the second-order form on the models, coordinates and scalers of a first-order form"""
    return propagate2_numpy_form(form.gps, form.coord, form.in_scaler, form.out)


# ---- 1. plumbing -------------------------------------------------------------------------------------------------------------------
def test_libgpk_exports_the_second_order_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        first = name.replace("propagate2", "propagate")
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.SIGNATURES[first][0] and len(args) == len(_lib.SIGNATURES[first][1]) + 2
        assert args[:-2] == _lib.SIGNATURES[first][1] and args[-2] is ctypes.c_int


def _surfaces():
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    from unmanned_aerial_vehicles_amd.sparse_batch import BatchedSparseGP
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    return ((pkg.GaussianProcessRegressor, "propagate"), (pkg.BatchedARDGP, "propagate"), (SparseGP, "propagate"),
            (BatchedSparseGP, "propagate"), (pkg.SimpleQuadrotorGP, "propagate_horizon"), (PreTrainedGP, "propagate_horizon"))


def test_order_is_on_the_six_surfaces():
    for cls, name in _surfaces():
        p = inspect.signature(getattr(cls, name)).parameters
        assert "order" in p and p["order"].default == 1, (cls, name)
    from unmanned_aerial_vehicles_amd.propagate import check_order, host_loop
    assert check_order(1) == 1 and check_order(2) == 2
    for bad in (0, 3, "2", 2.5, None, True):
        with pytest.raises(ValueError, match="order must be 1 or 2"):
            check_order(bad)
    assert inspect.signature(host_loop).parameters["hess_stage"].default is None


def test_order_3_is_a_value_error():
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    nx, D, H = 3, 5, 4
    x0, U, lin = np.zeros(nx), np.zeros((H, D - nx)), np.zeros((nx, D))
    # before the device and before the model is looked at: an unfitted estimator still names the order
    for obj in (pkg.GaussianProcessRegressor(), pkg.BatchedARDGP()):
        with pytest.raises(ValueError, match="order"):
            obj.propagate(x0, U, lin, order=3)
    state, Ug = np.arange(6.0) / 7.0, np.linspace(-1.0, 1.0, 12).reshape(4, 3)
    for obj in (pkg.SimpleQuadrotorGP(), PreTrainedGP(os.path.join(ROOT, "no_such_model_file.pkl"))):
        with pytest.raises(ValueError, match="order"):
            obj.propagate_horizon(state, Ug, 0.1, order=3)


# ---- the Hessian of the form against the committed fixture ------------------------------------------------------------------------
def test_closed_form_hessian_matches_the_fixture(csv_data):
    ref = np.load(os.path.join(GOLDEN, "hess_ref.npz"))
    g = gp_numpy_form(csv_data["X10"], csv_data["Y6"], 0.5, 1.0, 0.1, 1e-4)
    Xq = ref["ka1_Xq"][:8]
    e = relerr(closed_form_hessian(*mean_model(g), Xq), ref["ka1_hess"][:8])
    g1 = gp_numpy_form(csv_data["X10"], csv_data["Y6"][:, 0], 0.5, 1.0, 0.1, 1e-4, normalize=False)
    e1 = relerr(closed_form_hessian(*mean_model(g1), ref["one_Xq"][:8])[:, 0], ref["one_hess"][:8])
    print(f"closed-form Hessian against hess_ref.npz: ka1 {e:.2e}, one {e1:.2e} (bar 1e-8; the fixture's own fp64 check "
          f"{float(ref['ka1_chk']):.1e})")
    assert e < 1e-8 and e1 < 1e-8
    # and through the form's scalers: raw units, as make_golden_hess.py's case `axis` scales it
    form = propagate2_numpy_form([g1], [0], (np.full(10, 0.1), np.linspace(0.5, 2.0, 10)), ([0.3], [1.7]))
    q = ref["one_Xq"][:4] * form.in_scaler[1] + form.in_scaler[0]
    want = 1.7 * ref["one_hess"][:4] / (form.in_scaler[1][:, None] * form.in_scaler[1][None, :])
    assert relerr(form.hess(q)[:, 0], want) < 1e-8


# ---- 2. the order of the error ---------------------------------------------------------------------------------------------------
def _expected_next(form, x0, u, lin, F, nodes=14):
    """E[step(x)] for x ~ N(x0, F F^T), F (nx, k) with k = 1 or 2 columns: the tensor Gauss-Hermite rule on the factor's columns"""
    t, wt = np.polynomial.hermite.hermgauss(nodes)
    grid = np.stack(np.meshgrid(*([t] * F.shape[1]), indexing="ij"), axis=-1).reshape(-1, F.shape[1])
    wts = np.prod(np.stack(np.meshgrid(*([wt] * F.shape[1]), indexing="ij"), axis=-1).reshape(-1, F.shape[1]), axis=1)
    pts = x0[None, :] + np.sqrt(2.0) * grid @ F.T
    nxt = form.step(pts, np.tile(u, (len(pts), 1)), lin, False)[0]
    return (wts / np.pi ** (0.5 * F.shape[1])) @ nxt


@pytest.mark.parametrize("name", SINGLE_CASES)
def test_the_corrected_mean_is_second_order_accurate(name):
    c, form = single_form(name)
    form2 = second(form)
    lin, x0, u = c["lin"], c["x0"][0], c["U"][0]
    nx = lin.shape[0]
    V = np.linalg.qr(np.random.default_rng(0).standard_normal((nx, 2)))[0]
    errs = []
    for s in (6.25e-3, 1.5625e-3):
        S = s * V @ V.T
        S = 0.5 * (S + S.T)
        exact = _expected_next(form, x0, u, lin, np.sqrt(s) * V)
        t1 = form.run(x0[None], u[None, None], lin, S[None])[0][1, 0]
        t2, _, st = form2.run2(x0[None], u[None, None], lin, S[None])
        assert np.array_equal(t2[1, 0][form.coord], (t1[form.coord] + st["corr"][0, 0])), "c is added last, as one addition"
        errs.append((float(np.max(np.abs(exact - t1))), float(np.max(np.abs(exact - t2[1, 0])))))
    (f1, s1), (f2, s2) = errs
    print(f"case {name}: |E[x_1] - predicted|, first order {f1:.2e} / {f2:.2e} (falls {f1 / f2:.1f}x), with tr(H Sigma) / 2 "
          f"{s1:.2e} / {s2:.2e} (falls {s1 / s2:.1f}x); corrected {f2 / s2:.0f}x closer at the smaller s")
    assert s1 < f1 and s2 < f2
    assert s1 / s2 >= 8.0
    assert f1 / f2 <= 6.0


# ---- 3. nothing to correct without a covariance ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE_CASES)
def test_zero_covariance_leaves_the_first_stage_alone(name):
    c, form = single_form(name)
    x0, U = c["x0"][:1], c["U"][None]
    t1 = form.run(x0, U, c["lin"])[0]
    t2, S2, st = second(form).run2(x0, U, c["lin"])
    assert not st["corr"][0].any() and np.array_equal(t2[1], t1[1])
    assert st["corr"][1:].any(), "the model's own variance enters from the second stage on"


@pytest.mark.parametrize("name", SINGLE_CASES)
def test_second_order_cases_leave_room_under_the_bar(name):
    """What the 1e-8 bar of the GPU tests rests on at order 2: the growth of a 1e-12 relative perturbation of x0 along the horizon
    with the GPU tests' SPD Sigma0 and Q.  The corrected mean feeds Sigma back into x, so it grows far more than at order 1
    (4.8x): csv, H = 25, where Sigma reaches 3.6, measures 1.2e4x in x and 6.6e4x in corr here (R = 1; 5.9e4x and 1.4e5x over
    the GPU tests' five rollouts) - rounding differences of 1e-15 become 1e-10 there, which is what the GPU measures (2.6e-10) -
    and below 1e6x is what leaves the bar an order of magnitude.  The other cases stay below 2x."""
    c, form = single_form(name)
    form2 = second(form)
    nx = c["lin"].shape[0]
    S0, Q = spd(nx)
    x0, U = c["x0"][:1], c["U"][None]
    a = form2.run2(x0, U, c["lin"], S0[None], Q)
    b = form2.run2(x0 * (1.0 + 1e-12), U, c["lin"], S0[None], Q)
    gx, gs, gc = (relerr(b[0], a[0]) / 1e-12, relerr(b[1], a[1]) / 1e-12, relerr(b[2]["corr"], a[2]["corr"]) / 1e-12)
    print(f"case {name}, order 2, SPD Sigma0 and Q: growth of a 1e-12 perturbation of x0: {gx:.1f}x in x, {gs:.1f}x in Sigma, "
          f"{gc:.1f}x in corr; max |Sigma| {np.max(np.abs(a[1])):.2e}")
    assert max(gx, gs, gc) < 1e6


def test_host_loop_applies_the_correction_last():
    """`propagate.host_loop` with a second-order stage callback on the NumPy form: the form's own run2; without it, what it was."""
    from unmanned_aerial_vehicles_amd.propagate import host_loop
    c, form = single_form("b")
    form2 = second(form)
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    x0, U = c["x0"][:1], c["U"][None]

    def stage(q):
        return form.stage(q, False)

    a = host_loop(stage, form.coord, x0, U, lin, S0[None], Q, 1, U.shape[1])
    assert set(a[2]) == {"mean", "var", "jac"}
    w1 = form.run(x0, U, lin, S0[None], Q)
    assert relerr(a[0], w1[0]) < 1e-13 and relerr(a[1], w1[1]) < 1e-13
    b = host_loop(stage, form.coord, x0, U, lin, S0[None], Q, 1, U.shape[1], hess_stage=form2.hess)
    w2 = form2.run2(x0, U, lin, S0[None], Q)
    assert relerr(b[0], w2[0]) < 1e-13 and relerr(b[1], w2[1]) < 1e-13 and relerr(b[2]["corr"], w2[2]["corr"]) < 1e-12
    assert np.array_equal(b[0][1], a[0][1] + np.pad(b[2]["corr"][0], ((0, 0), (0, nx - form.NO))))


# ---- 4. the wrappers without a model ---------------------------------------------------------------------------------------------
def test_untrained_wrappers_return_the_nominal_horizon_at_order_2(capsys):
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    state, U, dt = np.arange(6.0) / 7.0, np.linspace(-1.0, 1.0, 12).reshape(4, 3), 0.1
    S0, Q = spd(6)
    sq = pkg.SimpleQuadrotorGP()
    pre = PreTrainedGP(os.path.join(ROOT, "no_such_model_file.pkl"))
    capsys.readouterr()
    for obj in (sq, pre):
        X, Sig = obj.propagate_horizon(state, U, dt, Sigma0=S0, process_noise=Q, order=2)
        said = capsys.readouterr().out
        assert "propagation" in said and ("not trained" in said or "no models are loaded" in said), said
        nominal, lin = nominal_rollouts(sq._nominal_dynamics, state, U, dt, 1)
        assert X.shape == (6, 4) and Sig.shape == (4, 6, 6)
        assert np.array_equal(X, nominal[0])
        assert np.allclose(Sig, _nominal_sigma(lin, S0, Q, 3), rtol=1e-14, atol=0)
    assert sq.prediction_count == 0
