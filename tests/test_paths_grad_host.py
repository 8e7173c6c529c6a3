"""Host-side checks of the path gradients ("path gradients"); no device is touched.

1. Plumbing: the six C entries are exported, declared and bound; the flag exists on the four classes and the two
   `sample_rollouts`; an untrained `SimpleQuadrotorGP` and a `PreTrainedGP` with nothing loaded return the nominal trajectory and
   a zero J.
2. The reference checks itself.  The closed-form NumPy Jacobian (`jac_numpy_form` and its batch and rollout forms in
   tests/test_gpu_paths_grad.py) against central differences of the NumPy value form, step 1e-5 of each input's scale, bar 1e-7
   of the largest component; and the product of the stage matrices I + lin_x + J_h over the horizon, applied to a random start
   perturbation, against central differences of the NumPy rollout at eps = 1e-6, bar 1e-6.  Measured (printed by the tests):
   Jacobian <= 6.1e-9 on the single cases, <= 7.1e-9 on the batch rollout cases, <= 2.9e-9 on the sparse cases (the input's
   scale is the standard deviation of the basis points' column, times in_scale for a raw-unit rollout); product <= 7.1e-9
   single, <= 2.9e-9 batch, <= 3.4e-9 sparse: every figure is under a tenth of its bar, and a wrong or missing term is of
   order one."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, relerr
from test_gpu_axis_paths import ROLLOUT_CASES, axis_paths_numpy_form, load_case as load_axis_case
from test_gpu_paths import CASE_NAMES, paths_numpy_form
from test_gpu_paths_grad import (FD_BAR, axis_rollout_jac_numpy_form, central_differences, input_scale, jac_numpy_form,
                                 rollout_jac_numpy_form)

NEW_SYMBOLS = ("gpk_paths_step_grad", "gpk_paths_rollout_grad", "gpk_paths_step_multi_grad", "gpk_paths_rollout_multi_grad",
               "gpk_paths_step_multi_grad_z", "gpk_paths_rollout_multi_grad_z")
PRODUCT_EPS, PRODUCT_BAR = 1e-6, 1e-6
SPARSE_SINGLE, SPARSE_ROLLOUT_BATCH = ("a", "b", "g"), ("c", "d", "e")


# ---- 1. plumbing -----------------------------------------------------------------------------------------------------------------------
def test_libgpk_exports_the_gradient_entries():
    from unmanned_aerial_vehicles_amd import _build, _lib
    assert os.path.exists(_build.LIB_PATH), "libgpk.so must be built in-tree (python __graft_entry__.py)"
    _lib.load()
    lib = ctypes.CDLL(_build.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert f"GPK_API int {name}(" in header
        value = name.replace("_grad", "")
        assert _lib.SIGNATURES[name][0] is _lib.SIGNATURES[value][0]
        rollout = "rollout" in name      # jac: device for a step, host for a rollout
        assert _lib.SIGNATURES[name][1] == _lib.SIGNATURES[value][1] + [_lib._dp if rollout else _lib._vp], name


def test_the_flag_exists_everywhere():
    import unmanned_aerial_vehicles_amd as pkg
    for cls in (pkg.PosteriorPaths, pkg.SparsePosteriorPaths, pkg.BatchedPosteriorPaths, pkg.BatchedSparsePosteriorPaths):
        for method in (cls.step, cls.rollout):
            assert inspect.signature(method).parameters["return_jacobian"].default is False, (cls, method)
    for cls in (pkg.SimpleQuadrotorGP, pkg.PreTrainedGP):
        assert inspect.signature(cls.sample_rollouts).parameters["return_jacobian"].default is False, cls
    assert pkg.BatchedSparsePosteriorPaths._STEP_GRAD == "gpk_paths_step_multi_grad_z"
    assert pkg.BatchedSparsePosteriorPaths._ROLLOUT_GRAD == "gpk_paths_rollout_multi_grad_z"


def test_untrained_models_return_the_nominal_trajectory_and_a_zero_jacobian(capsys):
    import unmanned_aerial_vehicles_amd as pkg
    state, U, dt, R = np.arange(6.0), np.ones((4, 3)), 0.1, 2
    sq = pkg.SimpleQuadrotorGP()
    X, J = sq.sample_rollouts(state, U, dt, n_rollouts=R, return_jacobian=True)      # untrained: nominal, no device
    assert X.shape == (R, 6, 4) and J.shape == (R, 3, 6, 10) and not J.any()
    assert np.array_equal(X, sq.sample_rollouts(state, U, dt, n_rollouts=R))
    pg = pkg.PreTrainedGP("/nonexistent/model.pkl")
    capsys.readouterr()
    X, J = pg.sample_rollouts(state, U, dt, n_rollouts=R, return_jacobian=True)
    assert "GP rollout sampling failed: no models are loaded" in capsys.readouterr().out
    assert X.shape == (R, 6, 4) and J.shape == (R, 3, 6, 10) and not J.any()
    assert np.array_equal(X, pg.sample_rollouts(state, U, dt, n_rollouts=R))


# ---- 2. the reference checks itself ----------------------------------------------------------------------------------------------------
def stage_product_error(rollout, A_of, x0, seed):
    """|prod_h A_h dx - central difference of the rollout's last stage along dx| / largest component, dx a random direction;
    rollout(x0) -> (H + 1, S, nx), A_of(traj) -> (H, S, nx, nx)"""
    S, nx = x0.shape
    dx = np.random.RandomState(seed).standard_normal((S, nx))
    traj = rollout(x0)
    v = dx.copy()
    for A in A_of(traj):
        v = np.einsum("sij,sj->si", A, v)
    fd = (rollout(x0 + PRODUCT_EPS * dx)[-1] - rollout(x0 - PRODUCT_EPS * dx)[-1]) / (2.0 * PRODUCT_EPS)
    return relerr(v, fd)


def single_checks(tag, form, Xb, c):
    S, P = form.V.shape[1:]
    scale = input_scale(Xb)
    e = relerr(jac_numpy_form(form, c["Xs"]), central_differences(form.step, c["Xs"], scale))
    print(f"{tag}: closed-form Jacobian against central differences of the value form: {e:.2e} (bar {FD_BAR:.0e})")
    assert e < FD_BAR
    lin, U = c["lin"], c["U"]
    x0 = np.broadcast_to(c["x0"], (S, P)).copy()
    A_of = lambda traj: np.eye(P) + lin[:, :P] + rollout_jac_numpy_form(form, traj, U)[:, :, :, :P]      # noqa: E731
    e = stage_product_error(lambda x: form.rollout(x, U, lin), A_of, x0, 5)
    print(f"{tag}: product of the stage matrices over {len(U)} stages against central differences of the rollout: {e:.2e} "
          f"(bar {PRODUCT_BAR:.0e})")
    assert e < PRODUCT_BAR


def batch_checks(tag, form, Xb, c):
    sc = (c["in"][0], c["in"][1])
    lin, U, coord = c["lin"], c["U"], c["coord"].astype(int)
    nx = lin.shape[0]
    S = form.forms[0].V.shape[1]
    x0 = np.broadcast_to(c["x0"], (S, nx)).copy()
    roll = lambda x: form.rollout(x, U, lin, coord, sc)      # noqa: E731
    traj = roll(x0)
    J = axis_rollout_jac_numpy_form(form, traj, U, sc)
    raw_scale = sc[1] * input_scale(Xb)
    worst = 0.0
    for h, u in enumerate(U):
        q = np.concatenate([traj[h], np.broadcast_to(u, (S, len(u)))], axis=1)
        worst = max(worst, relerr(J[h], central_differences(lambda Q: form.step((Q - sc[0]) / sc[1]), q, raw_scale)))
    print(f"{tag}: closed-form rollout Jacobian against central differences of the value form: {worst:.2e} (bar {FD_BAR:.0e})")
    assert worst < FD_BAR

    def A_of(tr):
        Jx = axis_rollout_jac_numpy_form(form, tr, U, sc)[:, :, :, :nx]
        A = np.broadcast_to(np.eye(nx) + lin[:, :nx], Jx.shape[:2] + (nx, nx)).copy()
        A[:, :, coord, :] += Jx
        return A

    e = stage_product_error(roll, A_of, x0, 6)
    print(f"{tag}: product of the stage matrices over {len(U)} stages against central differences of the rollout: {e:.2e} "
          f"(bar {PRODUCT_BAR:.0e})")
    assert e < PRODUCT_BAR


@pytest.mark.parametrize("name", CASE_NAMES)
def test_single_model_reference(name):
    d = np.load(os.path.join(GOLDEN, "paths_ref.npz"))
    c = {k[len(name) + 1:]: d[k] for k in d.files if k.startswith(name + "_")}
    sf2, noise, alpha = c["hyper"]
    form = paths_numpy_form(c["X"], c["Y"], c["ls"], sf2, noise, alpha, c["omega"], c["phase"], c["weights"], c["eps"])
    single_checks(f"case {name}", form, c["X"], c)


@pytest.mark.parametrize("name", ROLLOUT_CASES)
def test_batch_reference(name):
    c = load_axis_case(name)
    form = axis_paths_numpy_form(c["X"], c["Y"], c["ls"], c["hyper"], c["omega"], c["phase"], c["weights"], c["eps"], c["out"])
    batch_checks(f"batch case {name}", form, c["X"], c)


@pytest.fixture(scope="module")
def G():
    spec = importlib.util.spec_from_file_location("make_golden_sparse_paths", os.path.join(GOLDEN, "make_golden_sparse_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_sparse_case(name):
    d = np.load(os.path.join(GOLDEN, "sparse_paths_ref.npz"))
    return {k[len(name) + 1:]: d[k].astype(np.float64) for k in d.files if k.startswith(name + "_")}


@pytest.mark.parametrize("name", SPARSE_SINGLE + SPARSE_ROLLOUT_BATCH)
def test_sparse_reference(G, name):
    c = load_sparse_case(name)
    if name in SPARSE_SINGLE:
        form = G.SparseForm(c["Z"], c["X"], c["Y"], c["ls"], *c["hyper"], c["ynorm"][0], c["ynorm"][1], c["omega"], c["phase"],
                            c["weights"], c["xi"])
        single_checks(f"sparse case {name}", form, c["Z"], c)
    else:
        form = G.SparseBatchForm(c["Z"], c["X"], c["Y"], c["ls"], c["hyper"], c["ynorm"], c["omega"], c["phase"], c["weights"],
                                 c["xi"], c["out"])
        batch_checks(f"sparse batch case {name}", form, c["Z"].reshape(-1, c["Z"].shape[-1]), c)
