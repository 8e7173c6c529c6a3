"""tests/golden/sparse_train_ref.npz (the fixture of the sparse GP's training, written by
tests/golden/make_golden_sparse_train.py): the agreements it stores are within the bars its writer enforces and its gradients are
reproduced here by the dense N x N form; and the mapping between theta (the kernel's layout) and the `[ls .., noise, sf2]`
layout of `gpk_sparse_eval`, with fixed parameters and the isotropic sum.  NumPy / SciPy only: no GPU."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, relerr

FORMS_BAR = 1e-9      # the assembly form against the dense N x N form, of the largest component
CENTRAL_BAR = 1e-6    # central differences of the bound


def load_writer():
    spec = importlib.util.spec_from_file_location("make_golden_sparse_train", os.path.join(GOLDEN, "make_golden_sparse_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref():
    d = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    return {k: d[k] for k in d.files}


def test_stored_agreements_are_within_the_bars(ref):
    for case in ("A", "Aiso", "B"):
        forms, central = ref[case + "_agree"]
        print(f"case {case}: two forms {forms:.1e}, central differences {central:.1e}")
        assert 0.0 <= forms < FORMS_BAR and 0.0 <= central < CENTRAL_BAR
    assert 0.0 < float(ref["B_jitter_diff"]) < 1e-6
    assert float(ref["T_bound_opt"]) > float(ref["T_bound_start"])
    assert ref["A_X"].shape == (700, 4) and ref["A_Z"].shape == (130, 4) and ref["A_Y"].shape == (700, 2)
    assert ref["B_X"].shape == (300, 6) and ref["T_X"].shape == (600, 2) and ref["T_Z"].shape == (64, 2)
    assert ref["A_C"].shape == (132, 130) and ref["A_pass"].shape == (5,) and np.all(ref["A_pass_abs"] >= np.abs(ref["A_pass"]))


def test_gradients_by_the_dense_form(ref):
    w = load_writer()
    src = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    for k in ("A_X", "A_Y", "A_Z", "B_X", "B_Y"):
        assert np.array_equal(ref[k], src[k]), "cases A and B reuse the inputs of sparse_ref.npz"
    sf2, noise, alpha, jit = ref["A_hyper"]
    Yn = (ref["A_Y"] - ref["A_y_mean"]) / ref["A_y_std"]
    gd = w.grad_dense(ref["A_X"], Yn, ref["A_Z"], ref["A_ls"], sf2, noise, alpha, jit)
    assert relerr(ref["A_grad"], gd) < FORMS_BAR
    gi = w.grad_dense(ref["A_X"], Yn, ref["A_Z"], np.full(4, float(ref["Aiso_ls"][0])), sf2, noise, alpha, jit)
    assert relerr(ref["Aiso_grad"], np.concatenate([[gi[:4].sum()], gi[4:]])) < FORMS_BAR
    sf2, noise, alpha, jit = ref["B_hyper"]
    Yn = (ref["B_Y"] - ref["B_y_mean"]) / ref["B_y_std"]
    assert relerr(ref["B_grad"], w.grad_dense(ref["B_X"], Yn, ref["B_X"], ref["B_ls"], sf2, noise, alpha, jit)) < FORMS_BAR
    assert relerr(ref["B_grad"], ref["B_exact_grad"]) == pytest.approx(float(ref["B_jitter_diff"]))
    # the row pass's unweighted sum is 2 sum dL/dG o G + sum dL/dg o g
    sf2, noise, alpha, jit = ref["A_hyper"]
    Yn = (ref["A_Y"] - ref["A_y_mean"]) / ref["A_y_std"]
    _, unweighted, from_stats = w.grad_assembly(ref["A_X"], Yn, ref["A_Z"], ref["A_ls"], sf2, noise, alpha, jit)
    assert abs(unweighted - from_stats) < 1e-12 * abs(from_stats)


def test_theta_mapping():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    from unmanned_aerial_vehicles_amd.sparse import gradient_to_theta, hyper_from_theta
    g_ard = np.array([10.0, 20.0, 30.0, 4.0, 5.0])          # [ls_0, ls_1, ls_2, noise, sf2]
    g_iso = np.array([60.0, 4.0, 5.0])                      # [the features' sum, noise, sf2]
    # all free, ARD: theta = log [sf2, ls .., noise]
    k = ConstantKernel(2.0) * RBF([1.0, 2.0, 3.0]) + WhiteKernel(0.1)
    kern, comp, ls = hyper_from_theta(k, np.log([3.0, 0.5, 0.6, 0.7, 0.2]))
    assert np.allclose(ls, [0.5, 0.6, 0.7]) and np.isclose(comp.sf2, 3.0) and np.isclose(comp.noise, 0.2)
    assert np.array_equal(gradient_to_theta(comp, g_ard), [5.0, 10.0, 20.0, 30.0, 4.0])
    assert k.k1.k1.constant_value == 2.0, "the kernel passed in is left alone"
    # the noise fixed
    k = ConstantKernel(2.0) * RBF([1.0, 2.0, 3.0]) + WhiteKernel(0.1, noise_level_bounds="fixed")
    kern, comp, ls = hyper_from_theta(k, np.log([3.0, 0.5, 0.6, 0.7]))
    assert np.allclose(ls, [0.5, 0.6, 0.7]) and np.isclose(comp.sf2, 3.0) and comp.noise == 0.1
    assert np.array_equal(gradient_to_theta(comp, g_ard), [5.0, 10.0, 20.0, 30.0])
    # the constant fixed
    k = ConstantKernel(2.0, constant_value_bounds="fixed") * RBF([1.0, 2.0, 3.0]) + WhiteKernel(0.1)
    kern, comp, ls = hyper_from_theta(k, np.log([0.5, 0.6, 0.7, 0.2]))
    assert comp.sf2 == 2.0 and np.isclose(comp.noise, 0.2)
    assert np.array_equal(gradient_to_theta(comp, g_ard), [10.0, 20.0, 30.0, 4.0])
    # isotropic: one length-scale crosses the boundary, its gradient is the features' sum; no constant: sf2 = 1
    k = RBF(1.5) + WhiteKernel(0.1)
    kern, comp, ls = hyper_from_theta(k, np.log([0.4, 0.3]))
    assert ls.shape == (1,) and np.isclose(ls[0], 0.4) and comp.sf2 == 1.0 and np.isclose(comp.noise, 0.3)
    assert np.array_equal(gradient_to_theta(comp, g_iso), [60.0, 4.0])
    # no WhiteKernel, the length-scale fixed: only the constant is free
    k = ConstantKernel(2.0) * RBF(1.5, length_scale_bounds="fixed")
    kern, comp, ls = hyper_from_theta(k, np.log([7.0]))
    assert np.isclose(comp.sf2, 7.0) and ls[0] == 1.5 and comp.noise is None
    assert np.array_equal(gradient_to_theta(comp, g_iso), [5.0])
