"""Host-side checks of the gradient through exact moment matching (DESIGN.md, K11 "the adjoint of the moments"); no device is
touched.

`moments_vjp_numpy_form` below is the expected value of every GPU test of `predict_moments_vjp` and `propagate_moments_gradient`: a
dense NumPy adjoint of `moments_numpy_form` (tests/test_moments_host.py) that builds the N x N matrix L explicitly for every pair
of models, from R^-1 S itself, as that form does - another route than the kernels' (no factor of R^-1 S, no split exponent, no
tiles, both orders of a pair of models summed).

1. Plumbing: the four C entries are declared, bound and exported, the chain entries with their forward sibling's arity + 5; the
   package surface.
2. The form against central differences of `moments_numpy_form(dtype=np.longdouble)` in every component of the query and of its
   covariance (symmetric perturbations), on the cases a, b, one, csv of tests/golden/paths_ref.npz, the batch case gap of
   tests/golden/axis_paths_ref.npz (pairs of different models, scalers) and the 60-row synthetic model, at an SPD Sigma, and in
   the query at Sigma = 0.  The bar is not fixed in advance: 10 x the larger of the difference between the results at steps h and
   h / 2 and eps_longdouble |l| / h, both printed.
3. The horizon adjoint (`propagate.host_adjoint_moments` over the form) against central differences of `moments_numpy_form.run` in
   U, x0 and Sigma0 on case a by the same rule (`run` keeps float64 stages: its rounding is eps_float64 |l| / h); at Sigma0 = 0, H
   = 1 and gS = 0 it equals the linear `host_adjoint`'s dU and dx0 to rounding.
4. What the bar of the GPU tests rests on, printed and asserted: the float64 form within 1e-10 (of each array's largest component)
   of the same form in np.longdouble from the training data on, for the query batch on every case of the GPU tests (a, b, one,
   csv, big, wide; the batch cases a, gap, one, csv345) and for the horizon at the GPU tests' length, H = 4 stages (big and wide:
   their three).  Every E[v]
   stays above the floor on all of them (asserted along the horizon too): the clip is inactive, the cost is differentiable there.
5. The Python-side argument checks (before any device call) and the wrappers' fallback."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from test_moments_host import _inv, form_of, gaussian_query, moments_numpy_form, rel, synthetic
from test_propagate_host import axis_form, gp_numpy_form, spd

NEW_SYMBOLS = ("gpk_moments_vjp_host", "gpk_moments_vjp_host_multi", "gpk_propagate_mm_grad_host", "gpk_propagate_mm_grad_host_multi")
GPU_H = 4                                                 # stages of the GPU tests' horizons


class moments_vjp_numpy_form:
    """The adjoint of `moments_numpy_form.moments`, dense and in the form's own dtype: L is built explicitly for every pair of
    models, as the form builds it.

    .vjp(q (D,) raw, Sraw (nx, nx), noisy, gmean (NO,), gcov (NO, NO), gxcov (NO, D)) -> dq (D,), dS (nx, nx): the gradient of
    l = <gmean, mean> + <sym(gcov), V> + <gxcov[:, :nx], xcov[:, :nx]> with respect to the raw query and the raw covariance
    (entries taken as independent, the result symmetrised)."""

    def __init__(self, mform):
        self.f = mform

    def vjp(self, q, Sraw, noisy, gmean=None, gcov=None, gxcov=None):
        f = self.f
        dt = f.dt
        D, nx, NO = len(q), len(Sraw), f.NO
        shift, scale = (np.zeros(D), np.ones(D)) if f.in_scaler is None else f.in_scaler
        shift, scale = np.asarray(shift, dt), np.asarray(scale, dt)
        z = (np.asarray(q, dt) - shift) / scale
        S = np.zeros((D, D), dtype=dt)
        S[:nx, :nx] = np.asarray(Sraw, dt) / np.outer(scale[:nx], scale[:nx])
        I = np.eye(D, dtype=dt)
        ys = np.concatenate([g.ys for g in f.gps]).astype(dt)
        s = f.out[1].astype(dt) * ys
        eb = np.zeros(NO, dtype=dt) if gmean is None else np.asarray(gmean, dt) * s
        Vb = np.zeros((NO, NO), dtype=dt) if gcov is None else np.asarray(gcov, dt)
        Vb = (Vb + Vb.T) / 2 * np.outer(s, s)
        Cb = np.zeros((NO, D), dtype=dt)
        if gxcov is not None:
            Cb[:, :nx] = np.asarray(gxcov, dt)[:, :nx] * s[:, None] * scale[None, :nx]
        owner = [(g, p) for g, m in enumerate(f.model) for p in range(m[3].shape[1])]
        per = []
        for X, ls, sf2, a, _ in f.model:
            nu = X - z
            Binv, logdet = _inv(S + np.diag(ls ** 2))
            logdet -= np.sum(np.log(ls ** 2))
            per.append((nu, Binv, sf2 * np.exp(-logdet / 2 - np.einsum("nd,de,ne->n", nu, Binv, nu) / 2)))
        Emu = np.array([f.model[g][3][:, p] @ per[g][2] for g, p in owner])
        eh = eb - 2 * (Vb @ Emu)
        mbar, Sbar = np.zeros(D, dtype=dt), np.zeros((D, D), dtype=dt)
        for o, (g, p) in enumerate(owner):
            nu, Binv, l = per[g]
            beta = f.model[g][3][:, p] * l
            t = nu.T @ beta
            tb = Binv @ (S @ Cb[o])
            w = beta * (eh[o] + nu @ tb)
            Bnu = nu @ Binv
            mbar += Bnu.T @ w - tb * beta.sum()
            Sbar += (Bnu.T * w) @ Bnu / 2 - w.sum() / 2 * Binv + np.outer((I - Binv @ S) @ Cb[o], Binv @ t)
        kss = [dt.type(g.sf2 + (g.noise if noisy else 0.0)) for g in f.gps]
        for ga, (Xa, lsa, sfa, aa, Ka) in enumerate(f.model):
            for gb, (Xb, lsb, sfb, ab, _) in enumerate(f.model):
                oa = [o for o, w_ in enumerate(owner) if w_[0] == ga]
                ob = [o for o, w_ in enumerate(owner) if w_[0] == gb]
                Pa, Pb = 1 / lsa ** 2, 1 / lsb ** 2
                RiT, logR = _inv((S * (Pa + Pb)[None, :] + I).T)
                Mm = RiT.T @ S
                za, zb = (Xa - z) * Pa, (Xb - z) * Pb
                ea = np.log(sfa) - np.sum(za * (Xa - z), axis=1) / 2 + np.einsum("nd,de,ne->n", za, Mm, za) / 2
                eb_ = np.log(sfb) - np.sum(zb * (Xb - z), axis=1) / 2 + np.einsum("nd,de,ne->n", zb, Mm, zb) / 2
                L = np.exp(ea[:, None] + eb_[None, :] + za @ Mm @ zb.T - logR / 2)
                c = aa @ Vb[np.ix_(oa, ob)] @ ab.T
                if ga == gb:
                    Ev = kss[ga] - np.sum(Ka * L)
                    if Ev > 0:
                        c = c - np.trace(Vb[np.ix_(oa, oa)]) * Ka
                W = c * L
                wi, wj = W.sum(axis=1), W.sum(axis=0)
                A1 = za.T @ wi + zb.T @ wj
                cross = za.T @ W @ zb
                A2 = (za.T * wi) @ za + (zb.T * wj) @ zb + cross + cross.T
                mbar += RiT @ A1
                Sbar += RiT @ A2 @ RiT.T / 2 - W.sum() / 2 * (RiT * (Pa + Pb)[None, :])
        Sx = Sbar[:nx, :nx]
        return mbar / scale, (Sx + Sx.T) / 2 / np.outer(scale[:nx], scale[:nx])

    def batch(self, Q, Sraw, noisy, gmean=None, gcov=None, gxcov=None):
        """rows Q (M, D) -> dX (M, D), dSigma (M, nx, nx) as float64; seeds (M, ..) or None"""
        pick = lambda g, r: None if g is None else g[r]
        out = [self.vjp(q, s, noisy, pick(gmean, r), pick(gcov, r), pick(gxcov, r)) for r, (q, s) in enumerate(zip(Q, Sraw))]
        return tuple(np.array([o[i] for o in out], dtype=np.float64) for i in range(2))

    def stage_vjp(self, noisy):
        """the callback of `propagate.host_adjoint_moments`"""
        return lambda q, S, gm, gc, gxc: self.f.batch(q, S, noisy) + self.batch(q, S, noisy, gm, gc, gxc)

    def horizon(self, coord, x0, U, lin, Sigma0, Q, gx, gS, noisy=False):
        """traj, Sigma, dU, dx0, dSigma0 of the horizon: x0 (R, nx), U (R, H, nu), Sigma0 (R, nx, nx) or None"""
        from unmanned_aerial_vehicles_amd.propagate import host_adjoint_moments
        R, H = U.shape[0], U.shape[1]
        return host_adjoint_moments(lambda q, S: self.f.batch(q, S, noisy), self.stage_vjp(noisy), [int(c) for c in coord], x0, U, lin,
                                    Sigma0, Q, R, H, gx, gS)


def seeds(M, NO, D, seed=7):
    """random seeds of a query batch: (gmean (M, NO), gcov (M, NO, NO), not symmetric, gxcov (M, NO, D))"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((M, NO)), rng.standard_normal((M, NO, NO)), rng.standard_normal((M, NO, D))


def horizon_seeds(H, R, nx, seed=9):
    """random seeds of a horizon: gx (H + 1, R, nx), gS (H + 1, R, nx, nx), not symmetric"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((H + 1, R, nx)), rng.standard_normal((H + 1, R, nx, nx))


def fitted_data(name):
    """The arrays and hyper-parameters of the two models the GPU tests fit themselves (tests/test_gpu_moments.py: big, N = 333, and
    wide, nx = P = 10), from the same seeds: (c, ls, sf2, noise, alpha)."""
    if name == "big":
        rng = np.random.default_rng(333)
        N, D, P, H = 333, 5, 2, 3
        X = rng.standard_normal((N, D))
        Y = np.stack([0.3 * np.sin(X[:, 0] + X[:, 2]) + 0.1 * X[:, 4], 0.2 * np.cos(X[:, 1]) * X[:, 3]], axis=1)
        Y += 0.05 * rng.standard_normal((N, P))
        ls, sf2, noise, alpha = 1.5 + 0.2 * np.arange(D), 0.9, 0.02, 1e-8
        lin = 0.05 * rng.standard_normal((P, D))
        c = {"X": X, "Y": Y, "lin": lin, "x0": 0.3 * rng.standard_normal((1, P)), "U": 0.3 * rng.standard_normal((H, D - P))}
    else:
        rng = np.random.default_rng(1210)
        N, D, P, H = 70, 12, 10, 3
        X = rng.standard_normal((N, D))
        Y = 0.2 * np.sin(X @ rng.standard_normal((D, P)) / 2.0) + 0.03 * rng.standard_normal((N, P))
        ls, sf2, noise, alpha = 2.5 + 0.1 * np.arange(D), 0.8, 0.03, 1e-8
        c = {"X": X, "Y": Y, "lin": 0.03 * rng.standard_normal((P, D)), "x0": 0.3 * rng.standard_normal((1, P)),
             "U": 0.3 * rng.standard_normal((H, D - P))}
    return c, ls, sf2, noise, alpha


_forms = {}


def forms(name):
    """(arrays, float64 moments form, longdouble moments form, coord) of a case: "a", "b", "one", "csv" (paths_ref.npz), "big",
    "wide" (`fitted_data`), "axis:<case>" (axis_paths_ref.npz, csv345: the csv models 3..5 on coordinates 3, 4, 5), "synthetic";
    built once, shared, left unchanged"""
    if name in _forms:
        return _forms[name]
    if name.startswith("axis:"):
        c, pform = axis_form("csv", keep=(3, 4, 5), coord=(3, 4, 5)) if name == "axis:csv345" else axis_form(name[5:])
        ks = (3, 4, 5) if name == "axis:csv345" else range(len(pform.gps))
        for b, g in zip(ks, pform.gps):
            g.Yn = (c["Y"][:, b:b + 1] - g.ym) / g.ys
        out = (c, moments_numpy_form(pform.gps, pform.in_scaler, pform.out),
               moments_numpy_form(pform.gps, pform.in_scaler, pform.out, alpha=[c["hyper"][b][2] for b in ks], dtype=np.longdouble),
               list(pform.coord))
    elif name in ("big", "wide"):
        c, ls, sf2, noise, alpha = fitted_data(name)
        g = gp_numpy_form(c["X"], c["Y"], ls, sf2, noise, alpha)
        g.Yn = (c["Y"] - g.ym) / g.ys
        out = (c, moments_numpy_form([g]), moments_numpy_form([g], alpha=[alpha], dtype=np.longdouble), list(range(len(c["lin"]))))
    elif name == "synthetic":
        g = synthetic(1e-2)
        c = {"x0": np.array([[0.2, -0.3]]), "U": np.array([[0.4]]), "lin": np.zeros((2, 3))}
        out = (c, moments_numpy_form([g]), moments_numpy_form([g], alpha=[1e-10], dtype=np.longdouble), [0, 1])
    else:
        c, _, mform = form_of(name)
        out = (c, mform, form_of(name, np.longdouble)[2], list(range(c["lin"].shape[0])))
    _forms[name] = out
    return out


def query_of(c):
    q, S = gaussian_query(c)
    return q, S


def loss(form, q, S, gm, gc, gxc):
    nx = len(S)
    m, V, x, _ = form.moments(q, S, False)
    return np.sum(gm * m) + np.sum((gc + gc.T) / 2 * V) + np.sum(gxc[:, :nx] * x[:, :nx])


def central(f, h):
    return (f(h) - f(-h)) / (2 * h)


def by_the_step_rule(tag, got, fd, eps, scale):
    """got against the central differences fd(h) at h and h / 2: the bar is 10 x the larger of their difference and eps |l| / h"""
    h = 1e-4
    coarse, fine = fd(h), fd(h / 2)
    own = max(float(np.max(np.abs(coarse - fine))), float(eps * abs(scale) / h))
    err = float(np.max(np.abs(np.asarray(got, float) - fine)))
    print(f"{tag}: adjoint against central differences {err:.2e}; steps h and h / 2 differ by {np.max(np.abs(coarse - fine)):.2e}, "
          f"eps |l| / h = {eps * abs(scale) / h:.2e}; asserted against 10 x {own:.2e}  (largest component {np.max(np.abs(fine)):.2e})")
    assert err <= 10 * own, (tag, err, own)


# ---- 1. plumbing -------------------------------------------------------------------------------------------------------------------
def test_libgpk_exports_the_gradient_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES
    sig = _lib.SIGNATURES
    assert len(sig["gpk_propagate_mm_grad_host"][1]) == len(sig["gpk_propagate_mm_host"][1]) + 5
    assert len(sig["gpk_propagate_mm_grad_host_multi"][1]) == len(sig["gpk_propagate_mm_host_multi"][1]) + 5
    assert len(sig["gpk_moments_vjp_host"][1]) == len(sig["gpk_moments_host"][1]) + 5
    assert len(sig["gpk_moments_vjp_host_multi"][1]) == len(sig["gpk_moments_host_multi"][1]) + 5


def test_package_surface():
    import inspect
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd import propagate as pg
    from unmanned_aerial_vehicles_amd.device import DeviceGP
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    for cls in (pkg.GaussianProcessRegressor, pkg.BatchedARDGP):
        for fn in ("predict_moments_vjp", "propagate_moments_gradient"):
            assert callable(getattr(cls, fn, None)), (cls, fn)
        p = inspect.signature(cls.predict_moments_vjp).parameters
        assert [p[k].default for k in ("grad_mean", "grad_cov", "grad_xcov", "var_includes_noise")] == [None, None, None, False]
        p = inspect.signature(cls.propagate_moments_gradient).parameters
        assert p["route"].default == "auto" and p["grad_Sigma"].default is None
    for fn in (pkg.SimpleQuadrotorGP.horizon_gradient, PreTrainedGP.horizon_gradient):
        assert list(inspect.signature(fn).parameters)[-1] == "method" and inspect.signature(fn).parameters["method"].default == "linear"
    assert callable(pg.host_adjoint_moments) and callable(pg.check_moment_seeds)
    assert callable(DeviceGP.moments_vjp_host) and callable(DeviceGP.propagate_mm_grad_host)


# ---- 2. the form against central differences of the longdouble moments --------------------------------------------------------------
@pytest.mark.parametrize("zero", (False, True))
@pytest.mark.parametrize("name", ("a", "b", "one", "csv", "axis:gap", "synthetic"))
def test_form_matches_central_differences(name, zero):
    c, mform, lform, _ = forms(name)
    q, S = query_of(c)
    if name == "synthetic":
        S = np.array([[0.04, 0.01], [0.01, 0.03]])
    if zero:
        S = 0.0 * S
    D, nx, NO = len(q), len(S), mform.NO
    gm, gc, gxc = (s[0] for s in seeds(1, NO, D))
    dq, dS = moments_vjp_numpy_form(mform).vjp(q, S, False, gm, gc, gxc)
    assert dq.shape == (D,) and dS.shape == (nx, nx) and np.array_equal(dS, dS.T)
    eps = np.finfo(np.longdouble).eps
    l0 = float(loss(lform, q, S, gm, gc, gxc))
    fd_q = lambda h: np.array([float(central(lambda t: loss(lform, q + t * e, S, gm, gc, gxc), h)) for e in np.eye(D)])
    by_the_step_rule(f"{name}, Sigma {'= 0' if zero else 'SPD'}: dX", dq, fd_q, eps, l0)
    if zero:
        return      # (Sigma = 0 sits on the boundary of the PSD cone: no central difference in Sigma)

    def fd_S(h):
        out = np.zeros((nx, nx))
        for i in range(nx):
            for j in range(i + 1):
                E = np.zeros((nx, nx))
                E[i, j] = E[j, i] = 1.0
                d = float(central(lambda t: loss(lform, q, S + t * E, gm, gc, gxc), h))
                out[i, j] = out[j, i] = d if i == j else d / 2      # (the pair of entries moves together: dS_ij + dS_ji)
        return out
    by_the_step_rule(f"{name}, Sigma SPD: dSigma", dS, fd_S, eps, l0)


def test_seeds_of_none_are_zeros_and_the_seed_of_cov_is_symmetrised():
    c, mform, _, _ = forms("b")
    q, S = query_of(c)
    v = moments_vjp_numpy_form(mform)
    gm, gc, gxc = (s[0] for s in seeds(1, mform.NO, len(q)))
    a, b = v.vjp(q, S, False, gm, None, None), v.vjp(q, S, False, gm, 0 * gc, 0 * gxc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = v.vjp(q, S, False, None, gc, None), v.vjp(q, S, False, None, gc.T, None)
    assert rel(a[0], b[0]) <= 1e-14 and rel(a[1], b[1]) <= 1e-14
    assert not v.vjp(q, S, False)[0].any()


# ---- 3. the horizon adjoint ---------------------------------------------------------------------------------------------------------
def test_horizon_adjoint_matches_central_differences():
    c, mform, _, coord = forms("a")
    lin = c["lin"]
    nx, H = lin.shape[0], len(c["U"])
    S0, Q = spd(nx)
    S0 = 0.05 * S0
    x0, U = c["x0"][:1].copy(), c["U"][None].copy()
    gx, gS = horizon_seeds(H, 1, nx)
    v = moments_vjp_numpy_form(mform)
    traj, Sigma, dU, dx0, dS0 = v.horizon(coord, x0, U, lin, S0[None], Q, gx, gS)
    want = mform.run(coord, x0, U, lin, S0[None], Q)
    assert rel(traj, want[0]) <= 1e-13 and rel(Sigma, want[1]) <= 1e-13

    def cost(x0_, U_, S0_):
        t, s, _ = mform.run(coord, x0_, U_, lin, S0_[None], Q)
        return float(np.sum(gx * t) + np.sum((gS + gS.transpose(0, 1, 3, 2)) / 2 * s))

    eps, l0 = np.finfo(np.float64).eps, cost(x0, U, S0)

    def fd_U(h):
        out = np.zeros_like(U)
        for idx in np.ndindex(*U.shape):
            E = np.zeros_like(U)
            E[idx] = 1.0
            out[idx] = central(lambda t: cost(x0, U + t * E, S0), h)
        return out

    def fd_x(h):
        return np.array([[central(lambda t: cost(x0 + t * e[None], U, S0), h) for e in np.eye(nx)]])

    def fd_S(h):
        out = np.zeros((1, nx, nx))
        for i in range(nx):
            for j in range(i + 1):
                E = np.zeros((nx, nx))
                E[i, j] = E[j, i] = 1.0
                d = central(lambda t: cost(x0, U, S0 + t * E), h)
                out[0, i, j] = out[0, j, i] = d if i == j else d / 2
        return out

    by_the_step_rule("case a, horizon: dU", dU, fd_U, eps, l0)
    by_the_step_rule("case a, horizon: dx0", dx0, fd_x, eps, l0)
    by_the_step_rule("case a, horizon: dSigma0", dS0, fd_S, eps, l0)


@pytest.mark.parametrize("name", ("b", "csv"))
def test_at_zero_covariance_one_stage_is_the_linear_adjoint(name):
    """Sigma0 = 0, H = 1, gS = 0: the exact mean at a certain input is the posterior mean, so dU and dx0 are the linear sweep's"""
    from unmanned_aerial_vehicles_amd.propagate import host_adjoint
    c, pform, mform = form_of(name)
    lin = c["lin"]
    nx, D = lin.shape
    x0, U = c["x0"][:3], np.tile(c["U"][None, :1], (3, 1, 1))
    gx, _ = horizon_seeds(1, 3, nx)
    got = moments_vjp_numpy_form(mform).horizon(range(nx), x0, U, lin, None, None, gx, None)

    def stage(q):
        mean, jac, var = pform.stage(q, False)
        return mean, jac, var, np.zeros_like(jac)

    want = host_adjoint(stage, lambda q: np.zeros((3, nx, D, D)), list(range(nx)), x0, U, lin, None, None, 3, 1, gx, None)
    assert rel(got[0], want[0]) <= 1e-12
    assert rel(got[2], want[2]) <= 1e-12 and rel(got[3], want[3]) <= 1e-12


# ---- 4. conditioning: what the GPU bar rests on -------------------------------------------------------------------------------------
GPU_CASES = ("a", "b", "one", "csv", "big", "wide", "axis:a", "axis:gap", "axis:one", "axis:csv345")


@pytest.mark.parametrize("name", GPU_CASES)
def test_conditioning_of_the_query_batch(name):
    c, mform, lform, _ = forms(name)
    nx = c["lin"].shape[0]
    S0, _ = spd(nx)
    q = np.concatenate([c["x0"][0], c["U"][0]])
    S = 0.05 * S0
    gm, gc, gxc = (s[0] for s in seeds(1, mform.NO, len(q)))
    ev = mform.moments(q, S, False)[3]
    print(f"{name}: min E[v] = {float(np.min(ev)):.3e} (floor 0)")
    assert np.min(ev) > 0.0
    got = moments_vjp_numpy_form(mform).vjp(q, S, False, gm, gc, gxc)
    ext = moments_vjp_numpy_form(lform).vjp(q, S, False, gm, gc, gxc)
    for tag, a, b in zip(("dX", "dSigma"), got, ext):
        print(f"{name} {tag}: float64 against longdouble {rel(a, b):.2e}")
        assert rel(a, b) <= 1e-10, tag


@pytest.mark.parametrize("name", GPU_CASES)
def test_conditioning_of_the_horizon(name):
    c, mform, lform, coord = forms(name)
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    U = c["U"][None, :GPU_H]
    H = U.shape[1]
    x0 = c["x0"][:1]
    gx, gS = horizon_seeds(H, 1, nx)
    got = moments_vjp_numpy_form(mform).horizon(coord, x0, U, lin, 0.05 * S0[None], Q, gx, gS)
    ext = moments_vjp_numpy_form(lform).horizon(coord, x0, U, lin, 0.05 * S0[None], Q, gx, gS)
    for h in range(H):
        q = np.concatenate([got[0][h, 0], U[0, h]])
        ev = mform.moments(q, got[1][h, 0], False)[3]
        assert np.min(ev) > 0.0, (name, h)
    for tag, a, b in zip(("traj", "Sigma", "dU", "dx0", "dSigma0"), got, ext):
        print(f"{name}, H = {H}, {tag}: float64 against longdouble {rel(a, b):.2e}")
        assert rel(a, b) <= 1e-10, tag


# ---- 5. argument checks, before any device call -------------------------------------------------------------------------------------
def test_moment_seed_checks():
    from unmanned_aerial_vehicles_amd.propagate import check_moment_seeds
    gm, gc, gxc = check_moment_seeds(np.zeros((3, 2)), None, np.zeros((3, 2, 4)), 3, 2, 4)
    assert gm.shape == (3, 2) and gc is None and gxc.shape == (3, 2, 4)
    assert check_moment_seeds(np.zeros(2), np.zeros((2, 2)), None, 1, 2, 4)[1].shape == (1, 2, 2)
    for bad in ((np.zeros((3, 3)), None, None), (None, np.zeros((3, 2, 3)), None), (None, None, np.zeros((3, 2, 5))),
                (np.full((3, 2), np.nan), None, None), (None, np.full((3, 2, 2), np.inf), None), (np.zeros(2), None, None)):
        with pytest.raises(ValueError, match="predict_moments_vjp"):
            check_moment_seeds(*bad, 3, 2, 4)


def test_estimators_refuse_before_any_device_call():
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd import propagate as pg
    gp = pkg.GaussianProcessRegressor()
    with pytest.raises(RuntimeError, match="not fitted"):
        gp.predict_moments_vjp(np.zeros((1, 3)), np.eye(2))
    with pytest.raises(RuntimeError, match="not fitted"):
        gp.propagate_moments_gradient(np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), np.zeros((4, 1, 2)))
    with pytest.raises(RuntimeError, match="not fitted"):
        pkg.BatchedARDGP(optimizer=None).propagate_moments_gradient(np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), np.zeros((4, 1, 2)))
    # the unchanged refusal of the linear gradient chain, which now names the new method
    with pytest.raises(ValueError, match="propagate_gradient") as e:
        gp.propagate_gradient(np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), np.zeros((4, 1, 2)), method="moment")
    assert "propagate_moments_gradient" in str(e.value)
    # the checks the methods run, in their order: horizon, seeds, PSD, route
    x0, U, lin, S0, Q, R, H = pg.check_horizon(np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)), 2, 3, np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(ValueError, match="grad_traj"):
        pg.check_seeds(np.zeros((3, 1, 2)), None, R, H, 2)
    with pytest.raises(ValueError, match="NaN or infinity"):
        pg.check_seeds(np.full((4, 1, 2), np.nan), None, R, H, 2)
    with pytest.raises(ValueError, match="Sigma0 must be positive semi-definite"):
        pg.check_method("moment", 1, "propagate_moments_gradient", Sigma0=S0)
    with pytest.raises(ValueError, match="route must be"):
        pg.check_route("chain")


def test_fitted_estimators_check_their_arguments_first():
    import unmanned_aerial_vehicles_amd as pkg
    gp = pkg.GaussianProcessRegressor()
    gp.X_train_, gp._yn, gp.n_features_in_ = np.zeros((4, 3)), np.zeros((4, 2)), 3      # (no device model: a call past the checks fails)
    args = (np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="grad_traj"):
        gp.propagate_moments_gradient(*args, np.zeros((3, 1, 2)))
    with pytest.raises(ValueError, match="grad_Sigma"):
        gp.propagate_moments_gradient(*args, np.zeros((4, 1, 2)), np.zeros((4, 1, 2, 3)))
    with pytest.raises(ValueError, match="NaN or infinity"):
        gp.propagate_moments_gradient(*args, np.full((4, 1, 2), np.inf))
    with pytest.raises(ValueError, match="positive semi-definite"):
        gp.propagate_moments_gradient(*args, np.zeros((4, 1, 2)), Sigma0=np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(ValueError, match="route must be"):
        gp.propagate_moments_gradient(*args, np.zeros((4, 1, 2)), route="chain")
    with pytest.raises(ValueError, match="positive semi-definite"):
        gp.predict_moments_vjp(np.zeros((1, 3)), np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(ValueError, match="grad_cov"):
        gp.predict_moments_vjp(np.zeros((2, 3)), np.eye(2), grad_cov=np.zeros((2, 2, 3)))
    with pytest.raises(ValueError, match="grad_mean contains"):
        gp.predict_moments_vjp(np.zeros((2, 3)), np.eye(2), grad_mean=np.full((2, 2), np.nan))


def test_wrappers_fall_back(capsys):
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    sq = pkg.SimpleQuadrotorGP()
    gx = np.zeros((5, 6))
    gx[-1] = 1.0
    X, Sigma, dU, dx0 = sq.horizon_gradient(np.zeros(6), np.zeros((4, 4)), 0.05, gx, method="moment")
    assert X.shape == (6, 5) and Sigma.shape == (5, 6, 6) and dU.shape == (4, 4) and dx0.shape == (6,)
    assert "not trained" in capsys.readouterr().out
    plain = sq.horizon_gradient(np.zeros(6), np.zeros((4, 4)), 0.05, gx)
    assert all(np.array_equal(a, b) for a, b in zip((X, Sigma, dU, dx0), plain))
    # a sparse model has no gradient through its moments: the nominal fallback with the reason
    sq.gp_model, sq.is_trained = SparseGP.__new__(SparseGP), True
    again = sq.horizon_gradient(np.zeros(6), np.zeros((4, 4)), 0.05, gx, method="moment")
    out = capsys.readouterr().out
    assert "failed" in out and "SparseGP has no gradient through exact moments" in out
    assert all(np.array_equal(a, b) for a, b in zip(again, plain))
    pre = pkg.trainer.PreTrainedGP.__new__(pkg.trainer.PreTrainedGP)
    pre.is_loaded = False
    got = pre.horizon_gradient(np.zeros(6), np.zeros((4, 4)), 0.05, gx, method="moment")
    assert "failed" in capsys.readouterr().out and got[2].shape == (4, 4)
