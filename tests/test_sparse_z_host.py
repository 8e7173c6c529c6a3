"""tests/golden/sparse_z_ref.npz (the fixture of the gradient with respect to the inducing inputs, written by
tests/golden/make_golden_sparse_z.py): the agreements it stores are within the gates its writer enforces, the writer's two forms
and its central differences agree within the same gates on a fresh small draw, and the Python side of training Z - the
`[theta, Z.ravel()]` vector and the mapping of the two gradients into it, with fixed parameters and the isotropic kernel.  NumPy /
SciPy only: no GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

FORMS_GATE = 1e-6     # the assembly form against the dense N x N form, of the largest component
CENTRAL_GATE = 1e-5   # central differences of the bound


def load_z_writer():
    """make_golden_sparse_z.py as a module (it imports make_golden_sparse_train.py from its own folder)."""
    spec = importlib.util.spec_from_file_location("make_golden_sparse_z", os.path.join(GOLDEN, "make_golden_sparse_z.py"))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = path
    return mod


@pytest.fixture(scope="module")
def zref():
    d = np.load(os.path.join(GOLDEN, "sparse_z_ref.npz"))
    return {k: d[k] for k in d.files}


def test_stored_agreements_are_within_the_gates(zref):
    w = load_z_writer()
    assert (w.FORMS_GATE, w.FD_GATE) == (FORMS_GATE, CENTRAL_GATE) and w.FD_SAMPLE >= 12
    for case, shape in (("A", (130, 4)), ("Aiso", (130, 4)), ("T", (64, 2))):
        forms, central = zref[case + "_gradZ_agree"]
        print(f"case {case}: two forms {forms:.1e}, central differences {central:.1e}")
        assert 0.0 <= forms < FORMS_GATE and 0.0 <= central < CENTRAL_GATE
        assert zref[case + "_gradZ"].shape == shape and np.isfinite(zref[case + "_gradZ"]).all()
    assert zref["A_zpass"].shape == zref["A_zpass_abs"].shape == (130, 5)
    assert np.all(zref["A_zpass_abs"] >= np.abs(zref["A_zpass"]))
    # the training case: the two NumPy optima the issue quotes, and what separates them
    assert zref["Z16_Z"].shape == zref["Z16_z_opt_Z"].shape == (16, 2)
    assert abs(float(zref["Z16_bound_theta_opt"]) + 753.18) < 0.01 and abs(float(zref["Z16_bound_z_opt"]) + 546.79) < 0.01
    assert float(zref["Z16_bound_start"]) < float(zref["Z16_bound_theta_opt"]) < float(zref["Z16_bound_z_opt"])


def test_case_a_column_pass_matches_the_row_pass_fixture(zref):
    """Column 16 of the column pass summed over the inducing inputs is the row pass's unweighted sum, and the fixture's
    dL/dZ of case A is reproduced by the dense form."""
    w = load_z_writer()
    t = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    scale = float(t["A_pass_abs"][-1])
    assert abs(zref["A_zpass"][:, -1].sum() - float(t["A_pass"][-1])) < 1e-13 * scale
    assert abs(zref["A_zpass_abs"][:, -1].sum() - scale) < 1e-13 * scale
    sf2, noise, alpha, jit = t["A_hyper"]
    Yn = (t["A_Y"] - t["A_y_mean"]) / t["A_y_std"]
    gd = w.gradz_dense(t["A_X"], Yn, t["A_Z"], t["A_ls"], sf2, noise, alpha, jit)
    assert np.max(np.abs(gd - zref["A_gradZ"])) < FORMS_GATE * np.max(np.abs(zref["A_gradZ"]))


@pytest.mark.parametrize("iso", [False, True], ids=["ard", "isotropic"])
def test_two_forms_and_differences_on_a_fresh_draw(iso):
    w = load_z_writer()
    rng = np.random.default_rng(853)
    N, m, D, P = 90, 11, 3, 2
    X, Z, Yn = rng.uniform(-2.0, 2.0, (N, D)), rng.uniform(-2.0, 2.0, (m, D)), rng.standard_normal((N, P))
    ls = np.full(D, 0.8) if iso else np.array([0.7, 1.1, 0.9])
    g, forms, central = w.checked_gradz("fresh draw", X, Yn, Z, ls, 1.3, 0.07, 1e-8, 1e-6, 854)
    assert g.shape == (m, D) and forms < FORMS_GATE and central < CENTRAL_GATE
    # the column pass behind it: U from the coefficient matrix of the partial derivatives, and its unweighted column
    pt = w.W.partials(X, Yn, Z, ls, 1.3, 0.07, 1e-8, 1e-6)
    R, Ra = w.zpass_sums(X, Yn, Z, ls, 1.3, w.W.coef_matrix(pt))
    sums, asums = w.W.pass_sums(X, Yn, Z, ls, 1.3, w.W.coef_matrix(pt))
    assert abs(R[:, -1].sum() - sums[-1]) < 1e-13 * asums[-1]
    # ... and the expanded form T^T X - z sum T, which the library must not use, still agrees here (small sums)
    Kfu = w.W.rbf(X, Z, ls, 1.3)
    T = (np.hstack([Kfu, Yn]) @ w.W.coef_matrix(pt)) * Kfu
    expanded = T.T @ (X / ls) - (Z / ls) * T.sum(axis=0)[:, None]
    assert np.max(np.abs(expanded - R[:, :-1]) / Ra[:, :-1]) < 1e-13


def test_packing():
    from unmanned_aerial_vehicles_amd.sparse import pack_inducing, unpack_inducing
    theta = np.log([2.0, 0.5, 0.25])
    Z = np.arange(8.0).reshape(4, 2) - 3.5
    v = pack_inducing(theta, Z)
    assert v.shape == (11,) and np.array_equal(v[:3], theta) and np.array_equal(v[3:], Z.ravel())
    t2, Z2 = unpack_inducing(v, 3, (4, 2))
    assert np.array_equal(t2, theta) and np.array_equal(Z2, Z) and Z2.flags.c_contiguous
    t2[0], Z2[0, 0] = 99.0, 99.0
    assert v[0] == theta[0] and v[3] == Z[0, 0], "unpacking copies"
    with pytest.raises(ValueError):
        unpack_inducing(v, 2, (4, 2))
    with pytest.raises(ValueError):
        unpack_inducing(v[:-1], 3, (4, 2))


def test_gradient_mapping_beside_theta():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    from unmanned_aerial_vehicles_amd.sparse import gradient_to_theta, hyper_from_theta, pack_inducing

    def gradient_to_packed(comp, g, gZ):        # what train's objective does with log_bound's (grad_theta, grad_Z)
        return pack_inducing(gradient_to_theta(comp, g), gZ)

    gZ = np.array([[1.0, -2.0, 3.0], [4.0, 5.0, -6.0]])
    g_ard = np.array([10.0, 20.0, 30.0, 4.0, 5.0])          # [ls_0, ls_1, ls_2, noise, sf2]
    g_iso = np.array([60.0, 4.0, 5.0])                      # [the features' sum, noise, sf2]
    tail = [1.0, -2.0, 3.0, 4.0, 5.0, -6.0]
    # all free, ARD
    k = ConstantKernel(2.0) * RBF([1.0, 2.0, 3.0]) + WhiteKernel(0.1)
    comp = hyper_from_theta(k, k.theta)[1]
    assert np.array_equal(gradient_to_packed(comp, g_ard, gZ), [5.0, 10.0, 20.0, 30.0, 4.0] + tail)
    # the noise fixed; the constant fixed: theta's part shrinks, Z's part never does
    k = ConstantKernel(2.0) * RBF([1.0, 2.0, 3.0]) + WhiteKernel(0.1, noise_level_bounds="fixed")
    comp = hyper_from_theta(k, k.theta)[1]
    assert np.array_equal(gradient_to_packed(comp, g_ard, gZ), [5.0, 10.0, 20.0, 30.0] + tail)
    k = ConstantKernel(2.0, constant_value_bounds="fixed") * RBF([1.0, 2.0, 3.0]) + WhiteKernel(0.1)
    comp = hyper_from_theta(k, k.theta)[1]
    assert np.array_equal(gradient_to_packed(comp, g_ard, gZ), [10.0, 20.0, 30.0, 4.0] + tail)
    # isotropic: one length-scale in theta, but Z keeps a gradient per feature
    k = RBF(1.5) + WhiteKernel(0.1)
    comp = hyper_from_theta(k, k.theta)[1]
    out = gradient_to_packed(comp, g_iso, gZ)
    assert np.array_equal(out, [60.0, 4.0] + tail) and np.array_equal(out[:2], gradient_to_theta(comp, g_iso))
    # everything of the kernel fixed but the constant
    k = ConstantKernel(2.0) * RBF(1.5, length_scale_bounds="fixed")
    comp = hyper_from_theta(k, k.theta)[1]
    assert np.array_equal(gradient_to_packed(comp, g_iso, gZ), [5.0] + tail)


def test_new_keywords_exist():
    """The public surface this fixture is for (fails on a tree without the feature)."""
    import inspect
    from unmanned_aerial_vehicles_amd import SparseGP, _lib
    assert {"inducing", "eval_inducing_gradient"} <= set(inspect.signature(SparseGP.log_bound).parameters)
    assert inspect.signature(SparseGP.train).parameters["train_inducing"].default is False
    assert "gpk_sparse_eval_z" in _lib.SIGNATURES and "gpk_sparse_zgrad_pass" in _lib.SIGNATURES
