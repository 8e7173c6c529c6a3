"""Host-side checks of the gradient through exact moment matching on the sparse posteriors (DESIGN.md, K11 "the gradient on the
sparse models"); no device is touched.

The expected value of every GPU test of `SparseGP.predict_moments_vjp` / `propagate_moments_gradient` and their batch forms is
`moments_vjp_numpy_form(sparse_form(name))`: the dense NumPy adjoint of tests/test_moments_grad_host.py on the sparse moments form of
tests/test_sparse_moments_host.py ((Z, alpha_u, Q) per model) - the wrapper takes any moments form, so there is no new mathematics
here.  The problems are those of tests/test_sparse_propagate_host.py (single3, batch2, batch8, one200) with H = 4.

1. Plumbing: the four C entries are declared, bound and exported, each with five arguments more than its forward sibling; the
   package surface.
2. The sparse adjoint form against central differences of the np.longdouble sparse moments in every component of the query and of
   Sigma, at an SPD Sigma and (the query) at Sigma = 0, on single3, batch2 and one200, by `by_the_step_rule` of the exact host file:
   10 x the larger of the h vs h / 2 difference and eps |l| / h, both printed.
3. The horizon adjoint of single3 against central differences of the form's recursion in U, x0 and Sigma0, by the same rule.
4. What the bar of the GPU tests rests on - conditions the reference alone must meet: float64 against np.longdouble of the query
   adjoint and of the four-stage horizon on all four problems <= 1e-10 (the exact host file's bound), and min E[v] > 0 on every stage
   of every one of 32 rollouts, with and without Sigma0 / process noise: the clip is never active.
5. The Python-side argument checks (before any device call); the fallback of `model_moments_gradient` and of the wrappers."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from test_moments_grad_host import by_the_step_rule, central, horizon_seeds, loss, moments_vjp_numpy_form, seeds
from test_moments_host import rel
from test_propagate_host import rollouts, spd
from test_sparse_moments_host import _host_models, gaussian_rows, model_defs, sparse_form
from test_sparse_propagate_host import PROBLEMS, problem

NEW_SYMBOLS = {"gpk_sparse_moments_vjp": "gpk_sparse_moments", "gpk_sparse_moments_vjp_multi": "gpk_sparse_moments_multi",
               "gpk_sparse_propagate_mm_grad": "gpk_sparse_propagate_mm", "gpk_sparse_propagate_mm_grad_multi": "gpk_sparse_propagate_mm_multi"}
GPU_H = 4                                                 # stages of the GPU tests' horizons


def horizon_of(name, R, H=GPU_H):
    """the GPU tests' horizon of a problem: (x0 (R, nx), U (R, H, nu), Sigma0 (R, nx, nx), process noise (nx, nx))"""
    c = problem(name)[0]
    nx = c["lin"].shape[0]
    S0, Q = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"][:H], R)
    return x0, U, np.tile(0.05 * S0, (R, 1, 1)), Q


# ---- 1. plumbing -------------------------------------------------------------------------------------------------------------------
def test_libgpk_exports_the_sparse_gradient_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name, sibling in NEW_SYMBOLS.items():
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        assert name in _lib.SIGNATURES
        proto = header[header.index(f"GPK_API int {name}("):]
        proto = proto[:proto.index(");")]
        assert proto.count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[sibling][1]) + 5, name


def test_package_surface():
    import inspect
    from unmanned_aerial_vehicles_amd import propagate as pg
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    from unmanned_aerial_vehicles_amd.sparse_batch import BatchedSparseGP
    for cls in (SparseGP, BatchedSparseGP):
        for fn in ("predict_moments_vjp", "propagate_moments_gradient"):
            assert callable(getattr(cls, fn, None)), (cls, fn)
        p = inspect.signature(cls.predict_moments_vjp).parameters
        assert [p[k].default for k in ("grad_mean", "grad_cov", "grad_xcov", "var_includes_noise")] == [None, None, None, False]
        p = inspect.signature(cls.propagate_moments_gradient).parameters
        assert p["route"].default == "chain" and p["grad_Sigma"].default is None and p["var_includes_noise"].default is False
    for k in ("coord", "in_scaler", "out_scaler"):
        assert k in inspect.signature(BatchedSparseGP.propagate_moments_gradient).parameters
    for k in ("in_scaler", "out_scaler"):
        assert k in inspect.signature(BatchedSparseGP.predict_moments_vjp).parameters
    assert callable(pg.model_moments_gradient)


# ---- 2. the sparse adjoint form against central differences of the longdouble sparse moments ---------------------------------------
@pytest.mark.parametrize("zero", (False, True))
@pytest.mark.parametrize("name", ("single3", "batch2", "one200"))
def test_form_matches_central_differences(name, zero):
    mform, lform = sparse_form(name), sparse_form(name, np.longdouble)
    Qr, Sr = gaussian_rows(name, 1)
    q, S = Qr[0], Sr[0]
    if zero:
        S = 0.0 * S
    D, nx, NO = len(q), len(S), mform.NO
    gm, gc, gxc = (s[0] for s in seeds(1, NO, D))
    dq, dS = moments_vjp_numpy_form(mform).vjp(q, S, False, gm, gc, gxc)
    assert dq.shape == (D,) and dS.shape == (nx, nx) and np.array_equal(dS, dS.T)
    eps = np.finfo(np.longdouble).eps
    l0 = float(loss(lform, q, S, gm, gc, gxc))
    fd_q = lambda h: np.array([float(central(lambda t: loss(lform, q + t * e, S, gm, gc, gxc), h)) for e in np.eye(D)])  # noqa: E731
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


# ---- 3. the horizon adjoint ---------------------------------------------------------------------------------------------------------
def test_horizon_adjoint_matches_central_differences():
    name = "single3"
    c = problem(name)[0]
    mform, coord, lin = sparse_form(name), model_defs(name)[3], c["lin"]
    nx = lin.shape[0]
    x0, U, S0, Q = horizon_of(name, 1)
    S0 = S0[0]
    H = U.shape[1]
    gx, gS = horizon_seeds(H, 1, nx)
    traj, Sigma, dU, dx0, dS0 = moments_vjp_numpy_form(mform).horizon(coord, x0, U, lin, S0[None], Q, gx, gS)
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

    by_the_step_rule(f"{name}, horizon: dU", dU, fd_U, eps, l0)
    by_the_step_rule(f"{name}, horizon: dx0", dx0, fd_x, eps, l0)
    by_the_step_rule(f"{name}, horizon: dSigma0", dS0, fd_S, eps, l0)


# ---- 4. conditioning: what the GPU bar rests on -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_conditioning_of_the_query_adjoint(name):
    mform, lform = sparse_form(name), sparse_form(name, np.longdouble)
    Qr, Sr = gaussian_rows(name, 5)
    gm, gc, gxc = seeds(5, mform.NO, Qr.shape[1])
    for r in (0, 4):
        got = moments_vjp_numpy_form(mform).vjp(Qr[r], Sr[r], False, gm[r], gc[r], gxc[r])
        ext = moments_vjp_numpy_form(lform).vjp(Qr[r], Sr[r], False, gm[r], gc[r], gxc[r])
        for tag, a, b in zip(("dX", "dSigma"), got, ext):
            print(f"{name}, row {r} {tag}: float64 against longdouble {rel(a, b):.2e}")
            assert rel(a, b) <= 1e-10, (name, r, tag)


@pytest.mark.parametrize("name", PROBLEMS)
def test_conditioning_of_the_horizon(name):
    c = problem(name)[0]
    mform, lform, coord, lin = sparse_form(name), sparse_form(name, np.longdouble), model_defs(name)[3], c["lin"]
    nx = lin.shape[0]
    x0, U, S0, Q = horizon_of(name, 1)
    gx, gS = horizon_seeds(GPU_H, 1, nx)
    got = moments_vjp_numpy_form(mform).horizon(coord, x0, U, lin, S0, Q, gx, gS)
    ext = moments_vjp_numpy_form(lform).horizon(coord, x0, U, lin, S0, Q, gx, gS)
    for tag, a, b in zip(("traj", "Sigma", "dU", "dx0", "dSigma0"), got, ext):
        print(f"{name}, H = {GPU_H}, {tag}: float64 against longdouble {rel(a, b):.2e}")
        assert rel(a, b) <= 1e-10, (name, tag)


@pytest.mark.parametrize("name", PROBLEMS)
def test_the_clip_is_inactive_along_every_rollout(name):
    from test_sparse_moments_host import prior
    c = problem(name)[0]
    mform, coord, lin = sparse_form(name), model_defs(name)[3], c["lin"]
    x0, U, S0, Q = horizon_of(name, 32)
    pr = prior(name)
    for tag, args in (("Sigma0 and process noise", (S0, Q)), ("neither", (None, None))):
        traj, Sigma, _ = mform.run(coord, x0, U, lin, *args)
        share = min(float(np.min(mform.moments(np.concatenate([traj[h, r], U[r, h]]), Sigma[h, r], False)[3] / pr))
                    for h in range(GPU_H) for r in range(32))
        print(f"{name}, 32 rollouts, {GPU_H} stages, {tag}: min E[v] / prior {share:.3e}")
        assert share > 0.0, (name, tag)


# ---- 5. argument checks, before any device call; the fallback ----------------------------------------------------------------------
def test_estimators_check_their_arguments_before_any_device_call():
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    from unmanned_aerial_vehicles_amd.sparse_batch import BatchedSparseGP
    for cls in (SparseGP, BatchedSparseGP):
        with pytest.raises(RuntimeError, match="inducing inputs"):
            cls.predict_moments_vjp(cls.__new__(cls), np.zeros((1, 3)), np.eye(2))
        with pytest.raises(RuntimeError, match="inducing inputs"):
            cls.propagate_moments_gradient(cls.__new__(cls), np.zeros(1), np.zeros((3, 2)), np.zeros((1, 3)), np.zeros((4, 1, 1)))
    sp, bg = _host_models()
    bad = np.array([[1.0, 2.0], [2.0, 1.0]])
    for gp, NO in ((sp, 1), (bg, 2)):
        with pytest.raises(ValueError, match="predict_moments"):
            gp.predict_moments_vjp(np.zeros((2, 3)), bad)
        with pytest.raises(ValueError, match="M must be"):
            gp.predict_moments_vjp(np.zeros((33, 3)), np.eye(2))
        with pytest.raises(ValueError, match="grad_cov"):
            gp.predict_moments_vjp(np.zeros((2, 3)), np.eye(2), grad_cov=np.zeros((2, NO, NO + 1)))
        with pytest.raises(ValueError, match="grad_mean contains"):
            gp.predict_moments_vjp(np.zeros((2, 3)), np.eye(2), grad_mean=np.full((2, NO), np.nan))
        with pytest.raises(ValueError, match="grad_xcov"):
            gp.predict_moments_vjp(np.zeros((2, 3)), np.eye(2), grad_xcov=np.zeros((2, NO, 4)))
    # the single model: the state is its one output
    args = (np.zeros(1), np.zeros((3, 2)), np.zeros((1, 3)))
    with pytest.raises(ValueError, match="grad_traj"):
        sp.propagate_moments_gradient(*args, np.zeros((3, 1, 1)))
    with pytest.raises(ValueError, match="grad_Sigma"):
        sp.propagate_moments_gradient(*args, np.zeros((4, 1, 1)), np.zeros((4, 1, 1, 2)))
    with pytest.raises(ValueError, match="NaN or infinity"):
        sp.propagate_moments_gradient(*args, np.full((4, 1, 1), np.inf))
    with pytest.raises(ValueError, match="positive semi-definite"):
        sp.propagate_moments_gradient(*args, np.zeros((4, 1, 1)), Sigma0=-np.eye(1))
    with pytest.raises(ValueError, match="route must be"):
        sp.propagate_moments_gradient(*args, np.zeros((4, 1, 1)), route="auto")
    with pytest.raises(ValueError, match="R must be in"):
        sp.propagate_moments_gradient(np.zeros((33, 1)), args[1], args[2], np.zeros((4, 33, 1)))
    # the batch: nx = 2 of D = 3
    args = (np.zeros(2), np.zeros((3, 1)), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="grad_traj"):
        bg.propagate_moments_gradient(*args, np.zeros((4, 1, 3)))
    with pytest.raises(ValueError, match="route must be"):
        bg.propagate_moments_gradient(*args, np.zeros((4, 1, 2)), route="auto")
    with pytest.raises(ValueError, match="positive semi-definite"):
        bg.propagate_moments_gradient(*args, np.zeros((4, 1, 2)), process_noise=bad)
    with pytest.raises(ValueError, match="coord"):
        bg.propagate_moments_gradient(*args, np.zeros((4, 1, 2)), coord=(1, 1))
    with pytest.raises(ValueError, match="in_scale"):
        bg.propagate_moments_gradient(*args, np.zeros((4, 1, 2)), in_scaler=(np.zeros(3), np.zeros(3)))
    with pytest.raises(ValueError, match="in_scale"):
        bg.predict_moments_vjp(np.zeros((2, 3)), np.eye(2), in_scaler=(np.zeros(3), np.zeros(3)))


def test_a_model_that_cannot_serve_has_no_gradient_through_exact_moments(capsys):
    import unmanned_aerial_vehicles_amd as pkg
    from unmanned_aerial_vehicles_amd import propagate as pg
    from unmanned_aerial_vehicles_amd.sparse import SparseGP
    from unmanned_aerial_vehicles_amd.sparse_batch import BatchedSparseGP
    args = (np.zeros(6), np.zeros((4, 4)), np.zeros((6, 10)), np.zeros((5, 1, 6)), None)
    for cls in (SparseGP, BatchedSparseGP):
        with pytest.raises(ValueError, match=f"^{cls.__name__} has no gradient through exact moments") as e:
            pg.model_moments_gradient(cls.__new__(cls), *args)
        assert "inducing inputs" in str(e.value), "the reason follows"
    with pytest.raises(ValueError, match="^object has no gradient through exact moments"):
        pg.model_moments_gradient(object(), *args)
    # an argument the model refuses stays the model's own ValueError
    sp, _ = _host_models()
    with pytest.raises(ValueError, match="^propagate: "):
        pg.model_moments_gradient(sp, *args)
    # a PreTrainedGP without models falls back to the nominal sweep, and says so
    pre = pkg.trainer.PreTrainedGP.__new__(pkg.trainer.PreTrainedGP)
    pre.is_loaded = False
    gx = np.zeros((5, 6))
    gx[-1] = 1.0
    got = pre.horizon_gradient(np.zeros(6), np.zeros((4, 4)), 0.05, gx, method="moment")
    assert "failed" in capsys.readouterr().out and got[2].shape == (4, 4)
    assert all(np.array_equal(a, b) for a, b in zip(got, pre.horizon_gradient(np.zeros(6), np.zeros((4, 4)), 0.05, gx)))
