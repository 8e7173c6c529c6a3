"""The FITC sparse GP ("FITC") on the GPU against tests/golden/sparse_fitc_ref.npz (NumPy / SciPy, two independent
forms; inputs of cases A and B: sparse_ref.npz): the weighted statistics pass alone on every panel / slab form and both q_i
routes, the `SparseGP` class on cases A, B and C, every downstream serving route against the dense NumPy forms of the sparse host
tests fed (Z, alpha_u, Wuu, WSigma) from the fixture's FITC statistics, the likelihood on held rows, persistence, the batch and
the loaders, and the refusals.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL)."""
import ctypes as C
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky, solve_triangular

from conftest import GOLDEN, relerr

pytestmark = pytest.mark.gpu

ROUTE_BAR = 1e-12     # routes that differ in summation order only
FP64_BAR = 1e-8
_dp = C.POINTER(C.c_double)


def rbf(A, B, ls, sf2):
    d = (A / ls)[:, None, :] - (B / ls)[None, :, :]
    return sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))


@pytest.fixture(scope="module")
def ref():
    """the inputs (sparse_ref.npz; case C: the FITC fixture's own) and the FITC expectations under "F_" + key"""
    d = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    out = {k: d[k] for k in d.files}
    d = np.load(os.path.join(GOLDEN, "sparse_fitc_ref.npz"))
    for k in d.files:
        out[k if k[2:] in ("X", "Y", "Z", "Xq", "ls", "hyper", "y_mean", "y_std", "idx") else "F_" + k] = d[k]
    out["B_Z"] = out["B_X"]
    return out


def case_model(ref, case, approximation="fitc"):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    sf2, noise, alpha, jit = ref[case + "_hyper"]
    kern = ConstantKernel(sf2) * RBF(ref[case + "_ls"]) + WhiteKernel(noise)
    return SparseGP(kern, ref[case + "_Z"], alpha=float(alpha), jitter_uu=float(jit), y_mean=ref[case + "_y_mean"],
                    y_std=ref[case + "_y_std"], approximation=approximation)


def expected_std(ref, case):
    noise = ref[case + "_hyper"][1]
    return np.sqrt(ref["F_" + case + "_var"] + noise)[:, None] * ref[case + "_y_std"][None, :]


def rel1(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def inverse_factor(Z, ls, sf2, jit, mp):
    """Wuu = Luu^-1 of Kuu + jit I (NumPy), padded with the identity to mp x mp: the layout gpk_trtri writes"""
    m = len(Z)
    W = np.eye(mp)
    W[:m, :m] = solve_triangular(cholesky(rbf(Z, Z, ls, sf2) + jit * np.eye(m), lower=True), np.eye(m), lower=True)
    return W


def run_pass(ref, case, panel, slabs, fused, scale_w=1.0):
    """gpk_sparse_accumulate_fitc on a case's rows with NumPy's inverse factor (times scale_w) -> S (nt x nt tensor), the sum of
    log lambda, the weights"""
    import torch
    from unmanned_aerial_vehicles_amd.device import Backend
    be = Backend(0).set_options(sparse_panel=panel, sparse_slabs=slabs, fitc_fused=fused)
    X, Z, ls = ref[case + "_X"], ref[case + "_Z"], np.ascontiguousarray(ref[case + "_ls"])
    Yn = (ref[case + "_Y"] - ref[case + "_y_mean"]) / ref[case + "_y_std"]
    sf2, noise, alpha, jit = ref[case + "_hyper"]
    n, D, m, P = X.shape[0], X.shape[1], Z.shape[0], Yn.shape[1]
    mp = (m + 127) // 128 * 128
    nt = mp + 128
    dX, dY, dZ = be.upload(X), be.upload(Yn), be.upload(Z)
    dW = be.upload(scale_w * inverse_factor(Z, ls, sf2, jit, mp))
    S = torch.zeros((nt, nt), dtype=torch.float64, device=be.device)
    lam = torch.full((1,), 0.25, dtype=torch.float64, device=be.device)      # (the sum is ADDED to what the word holds)
    w = torch.full((n,), float("nan"), dtype=torch.float64, device=be.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with be.lock:
        be.bind_stream()
        be.check(be.lib.gpk_sparse_accumulate_fitc(be.h, p(dX), p(dY), n, p(dZ), m, D, P, ls.ctypes.data_as(_dp), float(sf2), p(S), nt,
                                                   p(dW), mp, float(noise + alpha), p(lam), p(w)))
        be.sync()
    out = (S.clone(), float(lam.cpu()[0]) - 0.25, w.cpu().numpy())
    be.lib.gpk_destroy(be.h)
    return out


# ---- 1. the weighted pass alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel,slabs", [(256, 0), (256, 1), (256, 5), (0, 0)])
def test_weighted_pass_case_a(ref, panel, slabs):
    import torch
    m, mp, P = 130, 256, 2
    res = {}
    for fused in (1, 0):
        S, lam, w = run_pass(ref, "A", panel, slabs, fused)
        assert torch.equal(S, S.T), "S must be symmetric bit for bit"
        S2, lam2, w2 = run_pass(ref, "A", panel, slabs, fused)
        assert torch.equal(S, S2) and lam == lam2 and np.array_equal(w, w2), "the same calls must give the same bits"
        S = S.cpu().numpy()
        G, g, yy = S[:m, :m], S[:m, mp:mp + P], np.diag(S)[mp:mp + P]
        e = (relerr(G, ref["F_A_G"]), relerr(g, ref["F_A_g"]), relerr(yy, ref["F_A_yy"]), rel1(lam, ref["F_A_loglam"]),
             relerr(w, ref["F_A_w"]))
        print(f"panel {panel} slabs {slabs} fused {fused}: G {e[0]:.2e} g {e[1]:.2e} yy {e[2]:.2e} sum log lambda {e[3]:.2e} w {e[4]:.2e}")
        assert max(e[:4]) < ROUTE_BAR
        assert e[4] < FP64_BAR      # (w_i = s2 / lambda_i: an error of q_i counts in units of s2, not of sf2)
        assert np.isfinite(S).all() and np.isfinite(w).all() and w.min() > 0.0 and w.max() <= 1.0
        assert not S[m:mp].any() and not S[mp + P:].any(), "the padding of S must stay zero"
        res[fused] = (G, g, yy, lam, w)
    e = [relerr(a, b) for a, b in zip(res[1][:3], res[0][:3])] + [rel1(res[1][3], res[0][3])]
    print(f"panel {panel} slabs {slabs}: fused against unfused {max(e):.2e}")
    assert max(e) < ROUTE_BAR


@pytest.mark.parametrize("fused", [1, 0])
def test_the_clip_at_zero(ref, fused):
    """An inverse factor scaled up by 1e-3 makes q_i exceed sf2 at the rows that are inducing inputs (case C): lambda_i = s2 and
    w_i = 1 EXACTLY there.  Expectation: NumPy on the same factor."""
    X, Z, ls, idx = ref["C_X"], ref["C_Z"], ref["C_ls"], ref["C_idx"]
    sf2, noise, alpha, jit = ref["C_hyper"]
    s2 = noise + alpha
    m, mp = len(Z), 128
    Yn = (ref["C_Y"] - ref["C_y_mean"]) / ref["C_y_std"]
    W = 1.001 * inverse_factor(Z, ls, sf2, jit, mp)[:m, :m]
    Kuf = rbf(Z, X, ls, sf2)
    resid = sf2 - np.sum((W @ Kuf) ** 2, axis=0)
    assert (resid[idx] < 0).all() and (resid > 0).sum() > 400, "the clip must be active at the inducing rows only"
    lam_i = s2 + np.maximum(resid, 0.0)
    want_w = s2 / lam_i
    S, lam, w = run_pass(ref, "C", 256, 0, fused, scale_w=1.001)
    S = S.cpu().numpy()
    assert (w[idx] == 1.0).all()
    e = (relerr(w, want_w), relerr(S[:m, :m], (Kuf * want_w) @ Kuf.T), relerr(S[:m, mp:mp + 1], (Kuf * want_w) @ Yn),
         rel1(lam, np.sum(np.log(lam_i))))
    print(f"fused {fused}: w {e[0]:.2e} G {e[1]:.2e} g {e[2]:.2e} sum log lambda {e[3]:.2e}")
    assert e[0] < FP64_BAR and max(e[1:]) < ROUTE_BAR


# ---- 2. / 3. the class on cases A and C ------------------------------------------------------------------------------------
def fit_pieces(gp, X, Y, pieces):
    r0 = 0
    for k in pieces:
        gp.partial_fit(X[r0:r0 + k], Y[r0:r0 + k])
        r0 += k
    return gp


@pytest.mark.parametrize("case,pieces", [("A", (700,)), ("A", (300, 399, 1)), ("C", (500,)), ("C", (200, 299, 1))])
def test_class_against_the_fixture(ref, case, pieces):
    gp = case_model(ref, case)
    assert gp.approximation_ == "fitc"
    X, Y, Xq = ref[case + "_X"], ref[case + "_Y"], ref[case + "_Xq"]
    fit_pieces(gp, X, Y if case == "A" else Y[:, 0], pieces)
    assert gp.n_rows_ == len(X)
    P = Y.shape[1]
    mean, std = gp.predict(Xq, return_std=True)          # 40 rows: the panel route
    mean, std = mean.reshape(len(Xq), P), std.reshape(len(Xq), P)
    e = (relerr(mean, ref["F_" + case + "_mean"]), relerr(std, expected_std(ref, case)), rel1(gp.bound(), ref["F_" + case + "_lik"]))
    print(f"case {case} pieces {pieces}: mean {e[0]:.2e} std {e[1]:.2e} likelihood {e[2]:.2e}")
    assert max(e) < FP64_BAR
    st = gp.statistics()
    assert rel1(st["log_lambda_sum"], ref["F_" + case + "_loglam"]) < FP64_BAR and st["n_rows"] == len(X)
    # the <= 32-row route against the panel route
    parts = [gp.predict(Xq[a:b], return_std=True) for a, b in ((0, 32), (32, 40))]
    sm = np.concatenate([q[0] for q in parts]).reshape(len(Xq), P)
    ss = np.concatenate([q[1] for q in parts]).reshape(len(Xq), P)
    e2 = (relerr(sm, mean), relerr(ss, std))
    print(f"case {case}: small against panel route: mean {e2[0]:.2e} std {e2[1]:.2e}")
    assert max(e2) < ROUTE_BAR
    assert max(relerr(sm, ref["F_" + case + "_mean"]), relerr(ss, expected_std(ref, case))) < FP64_BAR


def test_case_c_weights(ref):
    _, _, w = run_pass(ref, "C", 0, 0, 1)
    assert np.isfinite(w).all() and w.min() > 0.0 and w.max() <= 1.0
    assert np.max(np.abs(1.0 - w[ref["C_idx"]])) < 1e-6, "rows that coincide with an inducing input"
    assert relerr(w, ref["F_C_w"]) < FP64_BAR
    assert w.min() < 0.1, "rows far from every inducing input are down-weighted"


# ---- 4. case B: Z = X ------------------------------------------------------------------------------------------------------
def test_case_b(ref):
    X, y, Xq = ref["B_X"], ref["B_Y"][:, 0], ref["B_Xq"]
    sf2 = ref["B_hyper"][0]
    fitc = case_model(ref, "B").partial_fit(X, y)
    dtc = case_model(ref, "B", "dtc").partial_fit(X, y)
    fm, fs = fitc.predict(Xq, return_std=True)
    dm, ds = dtc.predict(Xq, return_std=True)
    e = (relerr(fm[:, None], ref["F_B_mean"]), relerr(fs[:, None], expected_std(ref, "B")), rel1(fitc.bound(), ref["F_B_lik"]))
    print(f"case B against the fixture: mean {e[0]:.2e} std {e[1]:.2e} likelihood {e[2]:.2e}")
    assert max(e) < FP64_BAR
    # against the DTC model on the same data: ten times what NumPy measured between the two (the fixture's B_vs_dtc)
    ys2 = ref["B_y_std"][0] ** 2
    got = (relerr(fm, dm), relerr(fs ** 2 / ys2 / sf2, ds ** 2 / ys2 / sf2), rel1(fitc.bound(), dtc.bound()))
    print("case B FITC against DTC: mean %.2e var/sf2 %.2e likelihood %.2e  (NumPy: %.2e %.2e %.2e)" % (got + tuple(ref["F_B_vs_dtc"])))
    for g, w in zip(got, ref["F_B_vs_dtc"]):
        assert g < 10.0 * w


# ---- 5. downstream routes on case A ----------------------------------------------------------------------------------------
class fitc_numpy_form:
    """The dense forms of the sparse posterior from (Z, alpha_u, Wuu, WSigma) computed from the FIXTURE's FITC statistics: the
    interface of `gp_numpy_form` (tests/test_propagate_host.py: .stage, ym, ys, sf2, noise) and the serving quantities of
    `numpy_form` (tests/test_gpu_sparse_serve.py)."""

    def __init__(self, ref, case="A"):
        Z, ls = ref[case + "_Z"], ref[case + "_ls"]
        sf2, noise, alpha, jit = ref[case + "_hyper"]
        G, g = ref["F_" + case + "_G"], ref["F_" + case + "_g"]
        m, s2 = len(Z), noise + alpha
        self.Z, self.ls, self.sf2, self.noise = Z, ls, sf2, noise
        self.ym, self.ys = ref[case + "_y_mean"], ref[case + "_y_std"]
        self.Wuu = solve_triangular(cholesky(rbf(Z, Z, ls, sf2) + jit * np.eye(m), lower=True), np.eye(m), lower=True)
        LB = cholesky(np.eye(m) + self.Wuu @ G @ self.Wuu.T / s2, lower=True)
        self.WS = solve_triangular(LB, self.Wuu, lower=True)
        self.au = self.Wuu.T @ cho_solve((LB, True), self.Wuu @ g / s2)
        self.Q = self.Wuu.T @ self.Wuu - self.WS.T @ self.WS

    def serve(self, Xq):
        """mean (M, P), y_var with the noise level (M, P), dmean (M, P, D), dvar (M, P, D), hess (M, P, D, D), cov (M, M, P)"""
        ku = rbf(self.Z, Xq, self.ls, self.sf2)                                         # (m, M)
        U = ((self.Z / self.ls)[None, :, :] - (Xq / self.ls)[:, None, :]) / self.ls       # (M, m, D): (z - x) / ls^2
        dl = -U * self.ls                                                                # (x - z) / ls
        ys2 = self.ys ** 2
        Qk = self.Q @ ku
        mean = self.ym + self.ys * (ku.T @ self.au)
        var = self.sf2 + self.noise - np.sum(ku * Qk, axis=0)
        dmean = np.einsum("jm,mjd,jp->mpd", ku, U, self.au) * self.ys[None, :, None]
        dvar = -2.0 * np.einsum("jm,mjd,jm->md", ku, U, Qk)
        D = Xq.shape[1]
        hess = np.einsum("jm,jp,mjde->mpde", ku, self.au, dl[:, :, :, None] * dl[:, :, None, :] - np.eye(D)[None, None])
        hess = hess * self.ys[None, :, None, None] / np.outer(self.ls, self.ls)[None, None]
        cov = rbf(Xq, Xq, self.ls, self.sf2) + self.noise * np.eye(len(Xq)) - ku.T @ Qk
        return mean, np.maximum(var, 0.0)[:, None] * ys2, dmean, dvar[:, None, :] * ys2[None, :, None], hess, cov[:, :, None] * ys2

    def stage(self, Zq, noisy):
        mean, var, dmean = self.serve(Zq)[:3]
        if not noisy:
            var = np.maximum(var - self.noise * self.ys[None, :] ** 2, 0.0)
        return mean, dmean, var


def moments_form(f):
    """`moments_numpy_form` (tests/test_moments_host.py) on (Z, alpha_u, Q) as `sparse_moments_numpy_form` supplies them"""
    from test_moments_host import moments_numpy_form
    mf = moments_numpy_form.__new__(moments_numpy_form)
    mf.dt = np.dtype(np.float64)
    mf.in_scaler = None
    mf.gps = [SimpleNamespace(sf2=f.sf2, noise=f.noise, ym=f.ym, ys=f.ys)]
    mf.NO = len(f.ym)
    mf.out = (np.zeros(mf.NO), np.ones(mf.NO))
    mf.model = [(f.Z, f.ls, np.float64(f.sf2), f.au, f.Q)]
    return mf


@pytest.fixture(scope="module")
def served_a(ref):
    gp = case_model(ref, "A").partial_fit(ref["A_X"], ref["A_Y"])
    return gp, fitc_numpy_form(ref)


def check(tag, got, want, bar=FP64_BAR):
    e = relerr(got, want)
    print(f"{tag}: {e:.2e}")
    assert np.shape(got) == np.shape(want) and e < bar, tag


def test_downstream_serving_routes(ref, served_a):
    gp, f = served_a
    Xq = ref["A_Xq"][:5]
    mean, var, dmean, dvar, hess, cov = f.serve(Xq)
    got = gp.predict_jacobian(Xq, return_var=True)
    for tag, a, b in zip(("mean", "dmean", "var", "dvar"), got, (mean, dmean, var, dvar)):
        check("predict_jacobian " + tag, a, b)
    gm, gd, gh = gp.predict_hessian(Xq)
    check("predict_hessian hess", gh, hess)
    check("predict_hessian dmean", gd, dmean)
    cm, cc = gp.predict(Xq, return_cov=True)
    check("predict(return_cov) mean", cm, mean)
    check("predict(return_cov) cov", cc, cov)


def test_downstream_moments_and_horizons(ref, served_a):
    from test_moments_grad_host import moments_vjp_numpy_form, seeds
    from test_propagate_host import propagate_numpy_form, rollouts, spd
    gp, f = served_a
    mf = moments_form(f)
    P, D, H, R = 2, 4, 3, 2
    rng = np.random.default_rng(311)
    S0, Qn = spd(P)
    Xq = ref["A_Xq"][:R]
    Sq = np.stack([S0 * (0.05 + 0.01 * r) for r in range(R)])
    got = gp.predict_moments(Xq, Sq)
    want = mf.batch(Xq, Sq, False)
    for tag, a, b in zip(("mean", "cov", "xcov"), got, want):
        check("predict_moments " + tag, a, b)
    gmn, gcv, gxc = seeds(R, P, D)
    got = gp.predict_moments_vjp(Xq, Sq, gmn, gcv, gxc)
    want = moments_vjp_numpy_form(mf).batch(Xq, Sq, False, gmn, gcv, gxc)
    check("predict_moments_vjp dX", got[3], want[0])
    check("predict_moments_vjp dSigma", got[4], want[1])
    # horizons: x = the P outputs, u = the remaining D - P coordinates
    lin = 0.05 * rng.standard_normal((P, D))
    x0, U = rollouts(0.3 * rng.standard_normal(P), 0.4 * rng.standard_normal((H, D - P)), R)
    traj, Sigma = gp.propagate(x0, U, lin, Sigma0=0.05 * S0, process_noise=Qn, route="chain")
    wt, wS, _ = propagate_numpy_form([f]).run(x0, U, lin, np.tile(0.05 * S0, (R, 1, 1)), Qn, False)
    check("propagate(chain) traj", traj, wt)
    check("propagate(chain) Sigma", Sigma, wS)
    traj, Sigma = gp.propagate_moments(x0, U, lin, Sigma0=0.05 * S0, process_noise=Qn, route="chain")
    wt, wS = mf.run(list(range(P)), x0, U, lin, np.tile(0.05 * S0, (R, 1, 1)), Qn, False)[:2]
    check("propagate_moments(chain) traj", traj, wt)
    check("propagate_moments(chain) Sigma", Sigma, wS)


def test_downstream_paths(ref, served_a):
    gp, f = served_a
    paths = gp.sample_paths(4, n_features=64, random_state=5)
    r = paths.randomness
    m, F, S, P = len(f.Z), 64, 4, 2
    scale = np.sqrt(2.0 * f.sf2 / F)
    PhiZ = scale * np.cos(f.Z @ r["omega"].T + r["phase"])
    w2, x2 = r["weights"].reshape(F, S * P), r["xi"].reshape(m, S * P)
    V = (np.tile(f.au, (1, S)) + f.WS.T @ x2 - f.Wuu.T @ (f.Wuu @ (PhiZ @ w2))).reshape(m, S, P)
    Qs = ref["A_Xq"][:S]
    k, c = rbf(Qs, f.Z, f.ls, f.sf2), np.cos(Qs @ r["omega"].T + r["phase"])
    want = f.ym + f.ys * (np.einsum("sn,nsp->sp", k, V) + np.einsum("sf,fsp->sp", c, scale * r["weights"]))
    check("sample_paths(4, 64).step", paths.step(Qs), want)


# ---- 6. the likelihood on held rows ----------------------------------------------------------------------------------------
def test_log_bound_on_held_rows(ref):
    from unmanned_aerial_vehicles_amd import SparseGP
    X, Y = ref["A_X"], ref["A_Y"]
    gp = case_model(ref, "A").hold(X, Y)
    assert rel1(gp.log_bound(), ref["F_A_lik"]) < FP64_BAR
    assert rel1(gp.log_bound(gp.kernel_.theta), ref["F_A_lik"]) < FP64_BAR
    theta2 = gp.kernel_.theta + np.array([0.2, -0.1, 0.05, 0.1, -0.15, 0.3])
    v2 = gp.log_bound(theta2)
    sf2, noise, alpha, jit = ref["A_hyper"]
    fresh = SparseGP(gp.kernel_, ref["A_Z"], alpha=float(alpha), jitter_uu=float(jit), y_mean=ref["A_y_mean"], y_std=ref["A_y_std"],
                     approximation="fitc").partial_fit(X, Y)
    assert np.allclose(fresh.kernel_.theta, theta2)
    e = (rel1(v2, fresh.bound()), relerr(gp.predict(ref["A_Xq"]), fresh.predict(ref["A_Xq"])))
    print(f"log_bound(theta2) against a fresh model: value {e[0]:.2e} mean {e[1]:.2e}")
    assert max(e) < ROUTE_BAR
    assert abs(v2 - float(ref["F_A_lik"])) > 1.0, "the second theta is another model"
    before = gp.statistics()
    for kw in (dict(eval_gradient=True), dict(eval_inducing_gradient=True), dict(inducing=ref["A_Z"], eval_inducing_gradient=True)):
        with pytest.raises(ValueError, match="FITC"):
            gp.log_bound(theta2, **kw)
    with pytest.raises(ValueError, match="FITC"):
        gp.train(X, Y)
    after = gp.statistics()
    assert all(np.array_equal(before[k], after[k]) for k in before)


# ---- 7. persistence --------------------------------------------------------------------------------------------------------
def test_pickle_round_trip_and_more_rows(ref):
    X, Y, Xq = ref["A_X"], ref["A_Y"], ref["A_Xq"]
    whole = fit_pieces(case_model(ref, "A"), X, Y, (300, 400))
    first = case_model(ref, "A").partial_fit(X[:300], Y[:300])
    back = pickle.loads(pickle.dumps(first))
    assert back.approximation_ == "fitc" and back.n_rows_ == 300 and "log_lambda_sum" in back.statistics()
    back.partial_fit(X[300:], Y[300:])
    a, b = whole.statistics(), back.statistics()
    for k in ("G", "g", "yy", "log_lambda_sum", "n_rows"):
        assert np.array_equal(a[k], b[k]), k
    for x, y in zip(whole.predict(Xq, return_std=True) + (whole.bound(),), back.predict(Xq, return_std=True) + (back.bound(),)):
        assert np.array_equal(x, y)


# ---- 8. the batch and the loaders --------------------------------------------------------------------------------------------
def test_mixed_batch_has_the_bits_of_its_models(ref):
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    X, y, Xq = ref["C_X"], ref["C_Y"][:, 0], ref["C_Xq"][:9]
    models = []
    for b, kind in enumerate(("fitc", "dtc", "fitc")):
        models.append(case_model(ref, "C", kind).partial_fit(X, y * (1.0 + 0.5 * b) + 0.1 * b))
    bg = BatchedSparseGP(models)
    assert bg.approximations_ == ["fitc", "dtc", "fitc"]
    mean, dmean, var, dvar = bg.predict_jacobian(Xq, return_var=True)
    for b, mdl in enumerate(models):
        om, od, ov, _ = mdl.predict_jacobian(Xq, return_var=True)
        assert np.array_equal(mean[:, b], om) and np.array_equal(var[:, b], ov) and np.array_equal(dmean[:, b], od), f"model {b}"


class Scaler:
    """what the trainer and the loader read of a StandardScaler"""

    def __init__(self, a):
        self.mean_, self.scale_ = a.mean(axis=0), a.std(axis=0)

    def transform(self, a):
        return (a - self.mean_) / self.scale_


def test_trainer_sparsify_save_and_serve(ref, tmp_path):
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor, RBF, ConstantKernel, WhiteKernel
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES, GPTrainer, PreTrainedGP
    rng = np.random.default_rng(77)
    n = 160
    X = rng.standard_normal((n, 10))
    Y = np.stack([np.sin(X[:, i]) + 0.3 * X[:, (i + 1) % 10] + 0.05 * rng.standard_normal(n) for i in range(6)], axis=1)
    tr = GPTrainer(model_dir=str(tmp_path))
    sx = Scaler(X)
    for i, name in enumerate(OUTPUT_NAMES):
        sy = Scaler(Y[:, i:i + 1])
        kern = ConstantKernel(1.0) * RBF(np.full(10, 2.0)) + WhiteKernel(0.05)
        tr.gp_models[name] = GaussianProcessRegressor(kernel=kern, alpha=1e-8, normalize_y=True, optimizer=None).fit(
            sx.transform(X[:80]), sy.transform(Y[:80, i:i + 1]).ravel())
        tr.scalers_X[name], tr.scalers_y[name] = sx, sy
    tr.sparsify(X, Y, 24, approximation="fitc")
    assert all(m.approximation_ == "fitc" and m.n_rows_ == n for m in tr.gp_models.values())
    want = {name: m.predict(sx.transform(X[:3]), return_std=True) for name, m in tr.gp_models.items()}
    pre = PreTrainedGP(tr.save_models("fitc_models"))
    assert pre.is_loaded and pre.approximations_ == {name: "fitc" for name in OUTPUT_NAMES}
    mean, std = pre.predict_residual_batch(X[:3])
    assert np.isfinite(mean).all() and np.isfinite(std).all() and (std < 1e5).all()
    for i, name in enumerate(OUTPUT_NAMES):
        sy = tr.scalers_y[name]
        assert relerr(mean[:, i], want[name][0] * sy.scale_[0] + sy.mean_[0]) < FP64_BAR
        assert relerr(std[:, i], want[name][1] * sy.scale_[0]) < FP64_BAR


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_statistics_alone(ref):
    from unmanned_aerial_vehicles_amd import _lib
    X, Y = ref["A_X"], ref["A_Y"]
    gp = case_model(ref, "A").hold(X[:300], Y[:300])
    be = gp._backend()
    before = gp.statistics()
    ls = np.ascontiguousarray(ref["A_ls"])
    sf2, noise = ref["A_hyper"][:2]
    b, info = C.c_double(0.0), C.c_int(0)
    g, gZ = np.zeros(len(ls) + 2), np.zeros(ref["A_Z"].shape)
    p = _lib.host_ptr
    with be.lock:
        be.bind_stream()
        rc = be.lib.gpk_sparse_set_approximation(be.h, 0, C.byref(info))
        msg = be.lib.gpk_last_error(be.h).decode()
        assert rc == _lib.GPK_BAD_ARG and "rows" in msg, msg
        assert be.lib.gpk_sparse_set_approximation(be.h, 1, C.byref(info)) == _lib.GPK_OK       # repeating the kind is fine
        for call in (lambda: be.lib.gpk_sparse_eval(be.h, p(ls), len(ls), float(sf2), float(noise), C.byref(b), p(g), C.byref(info)),
                     lambda: be.lib.gpk_sparse_eval_z(be.h, None, p(ls), len(ls), float(sf2), float(noise), C.byref(b), None, p(gZ),
                                                      C.byref(info)),
                     lambda: be.lib.gpk_sparse_eval_z(be.h, p(ref["A_Z"]), p(ls), len(ls), 2.0 * float(sf2), float(noise), C.byref(b),
                                                      p(g), p(gZ), C.byref(info))):
            rc = call()
            msg = be.lib.gpk_last_error(be.h).decode()
            assert rc == _lib.GPK_BAD_ARG and "FITC" in msg, msg
    after = gp.statistics()
    assert all(np.array_equal(before[k], after[k]) for k in before), "a refused call must change nothing"
    assert not g.any() and not gZ.any() and b.value == 0.0
    # the object still evaluates and serves
    assert np.isfinite(gp.log_bound(gp.kernel_.theta)) and np.isfinite(gp.predict(ref["A_Xq"][:3])).all()
