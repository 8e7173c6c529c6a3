"""Horizon propagation of the per-axis batch on the GPU: `BatchedARDGP.propagate` (one C call,
`gpk_propagate_host_multi`) and `PreTrainedGP.propagate_horizon`, in raw units.  Buffers start out as NaN (conftest:
GPK_DEBUG_FILL).

Expected values: `propagate_numpy_form` of tests/test_propagate_host.py, one dense NumPy posterior per model with the input
scaler, the output scaler and the coordinate map around them.  Bar: the project's fp64 bar, 1e-8 of each array's largest
component; tests/test_propagate_host.py prints and asserts what it rests on for every case used here (variance / prior >= 0.7 %,
growth of a 1e-12 perturbation of x0 at most 46x in Sigma: csv, H = 25).  Bit identity is asserted with np.array_equal.

Inputs: tests/golden/axis_paths_ref.npz, cases (N, D, B, nx, H) = a (120, 4, 2, 3, 6), csv (200, 10, 6, 6, 25), gap (96, 10, 4, 6,
5; coord = (0, 2, 3, 5)), one (128, 3, 1, 2, 4), each behind its input and output scaler; csv's models 3..5 alone on coord =
(3, 4, 5) with nx = 6; `eight_problem` (64, 10, 8, 8, 6), seeded; the reference trainer's six models of
tests/golden/trainer_ref.npz behind `PreTrainedGP`."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, reference_pickle_dict
from test_gpu_axis_paths import fit_batch, load_case
from test_gpu_paths import check
from test_gpu_sparse_batch import model_dict  # noqa: F401  (the fixture: six sparse models behind one input scaler)
from test_gpu_propagate import check_all
from test_propagate_host import (axis_form, eight_problem, reference_horizon, reference_models_form, rollouts, sparse_batch_problem,
                                 spd)

pytestmark = pytest.mark.gpu

_batches = {}


def batch(name, keep=None):
    """the fitted batch of a case (the models `keep`, default all): built once, shared, left unchanged"""
    key = (name, None if keep is None else tuple(keep))
    if key not in _batches:
        c = eight_problem()[0] if name == "eight" else load_case(name)
        _batches[key] = fit_batch(c, keep)
    return _batches[key]


def problem(name):
    """(arrays, batch, NumPy form, keyword arguments of `propagate`) of a parity case"""
    if name == "eight":
        c, form = eight_problem()
        bg, coord, out = batch("eight"), c["coord"], c["out"]
    elif name == "csv345":
        c, form = axis_form("csv", keep=(3, 4, 5), coord=(3, 4, 5))
        bg, coord, out = batch("csv", (3, 4, 5)), (3, 4, 5), c["out"][:, 3:6]
    else:
        c, form = axis_form(name)
        bg, coord, out = batch(name), c["coord"], c["out"]
    return c, bg, form, dict(coord=coord, in_scaler=(c["in"][0], c["in"][1]), out_scaler=(out[0], out[1]))


# ---- 1. parity with the NumPy form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("a", "csv", "csv345", "gap", "one", "eight"))
def test_parity_with_the_numpy_form(name):
    c, bg, form, kw = problem(name)
    lin = c["lin"]
    nx, H, B = lin.shape[0], len(c["U"]), len(bg.models)
    S0, Q = spd(nx)
    for R in (1, 5):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        for noisy in (False, True):
            got = bg.propagate(x0, U, lin, var_includes_noise=noisy, return_stages=True, **kw)
            assert got[0].shape == (H + 1, R, nx) and got[1].shape == (H + 1, R, nx, nx) and got[2]["jac"].shape == (H, R, B, lin.shape[1])
            assert np.array_equal(got[0][0], x0) and not got[1][0].any()
            check_all(f"batch {name}, R = {R}, noise {noisy}, Sigma0 = 0", got, form.run(x0, U, lin, noisy=noisy))
        got = bg.propagate(x0, U, lin, Sigma0=S0, process_noise=Q, return_stages=True, **kw)
        check_all(f"batch {name}, R = {R}, SPD Sigma0 and Q", got, form.run(x0, U, lin, np.tile(S0, (R, 1, 1)), Q))
        Sigma = got[1]
        assert np.array_equal(Sigma, Sigma.transpose(0, 1, 3, 2)), "every Sigma[h, r] equals its transpose bit for bit"
    # a coordinate without a model advances by lin alone and receives no variance
    free = [i for i in range(nx) if i not in list(kw["coord"])]
    if free:
        traj, Sigma = bg.propagate(c["x0"][0], c["U"], lin, **kw)
        q0 = np.concatenate([c["x0"][0], c["U"][0]])
        assert np.allclose(traj[1, 0, free], (c["x0"][0] + lin @ q0)[free], rtol=1e-14, atol=0)
        assert not Sigma[1, 0][free][:, free].any()


# ---- 2. the bits of predict_host_grad at the returned rows; the bits of the single-model entry --------------------------------
@pytest.mark.parametrize("name,R", [("a", 1), ("a", 16), ("a", 17), ("a", 32), ("csv", 17), ("eight", 5)])
def test_stage_outputs_have_the_bits_of_predict_host_grad(name, R):
    c, bg, _, kw = problem(name)
    Uc = c["U"][:4]
    x0, U = rollouts(c["x0"][0], Uc, R)
    traj, Sigma, st = bg.propagate(x0, U, c["lin"], coord=kw["coord"], var_includes_noise=True, return_stages=True)
    for h in range(len(Uc)):
        q = np.ascontiguousarray(np.concatenate([traj[h], U[:, h]], axis=1))
        mean, dmean, var, _ = bg.predict_host_grad(q, return_var=True)
        assert np.array_equal(st["mean"][h], mean), (name, R, h, "mean")
        assert np.array_equal(st["jac"][h], dmean), (name, R, h, "jac")
        assert np.array_equal(st["var"][h], var), (name, R, h, "var")


def test_one_model_has_the_bits_of_the_single_model_entry():
    c = load_case("one")
    bg = batch("one")
    gp = bg.models[0]
    D = c["lin"].shape[1]
    lin = np.ascontiguousarray(c["lin"][:1])                      # a state of one coordinate: nx = P = 1, two controls
    x0 = c["x0"][0][:1]
    U = np.concatenate([c["U"], 0.5 * c["U"][::-1]], axis=1)
    assert U.shape[1] == D - 1
    S0, Q = spd(1)
    for noisy in (False, True):
        a = bg.propagate(x0, U, lin, Sigma0=S0, process_noise=Q, var_includes_noise=noisy, return_stages=True)
        b = gp.propagate(x0, U, lin, Sigma0=S0, process_noise=Q, var_includes_noise=noisy, return_stages=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for k in ("mean", "var", "jac"):
            assert np.array_equal(a[2][k], b[2][k]), k


# ---- 3. the same bits every call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("a", "csv", "eight"))
def test_repeatable(name):
    c, bg, _, kw = problem(name)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    a = bg.propagate(x0, U, c["lin"], return_stages=True, **kw)
    b = bg.propagate(x0, U, c["lin"], return_stages=True, **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in ("mean", "var", "jac"):
        assert np.array_equal(a[2][k], b[2][k]), k


# ---- 4. the host-loop route ---------------------------------------------------------------------------------------------------------
def test_host_loop_route_agrees():
    c, bg, _, kw = problem("gap")
    x0, U = rollouts(c["x0"][0], c["U"], 3)
    S0, Q = spd(6)
    for noisy in (False, True):
        args = dict(Sigma0=S0, process_noise=Q, var_includes_noise=noisy, return_stages=True, **kw)
        check_all(f"batch gap, route = host, noise {noisy}", bg.propagate(x0, U, c["lin"], route="host", **args),
                  bg.propagate(x0, U, c["lin"], **args))


def test_sparse_batch_takes_the_host_loop():
    """`BatchedSparseGP.propagate`: the arguments of `BatchedARDGP.propagate`, the recursion as a host loop over the batch's
    `predict_jacobian`, against the NumPy form on the dense form of the sparse posteriors."""
    from test_gpu_sparse_batch import case
    c, form = sparse_batch_problem()
    bg = case(2, 60, 400, 10)[2]
    kw = dict(coord=c["coord"], in_scaler=(c["in"][0], c["in"][1]), out_scaler=(c["out"][0], c["out"][1]))
    x0, U = rollouts(c["x0"][0], c["U"], 3)
    S0, Q = spd(6)
    for noisy in (False, True):
        got = bg.propagate(x0, U, c["lin"], Sigma0=S0, process_noise=Q, var_includes_noise=noisy, return_stages=True, **kw)
        assert got[0].shape == (6, 3, 6) and got[1].shape == (6, 3, 6, 6) and got[2]["jac"].shape == (5, 3, 2, 10)
        check_all(f"two sparse models, noise {noisy}", got, form.run(x0, U, c["lin"], np.tile(S0, (3, 1, 1)), Q, noisy=noisy))
    a, b = bg.propagate(x0, U, c["lin"], route="host", **kw), bg.propagate(x0, U, c["lin"], **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        bg.propagate(x0, U, c["lin"], route="device", **kw)
    with pytest.raises(ValueError):
        bg.propagate(x0, U, c["lin"][:1], **kw)                 # nx = 1 < B


# ---- 5. the trainer's wrapper, in raw units --------------------------------------------------------------------------------------
def _ref_pre(trainer_ref):
    from unmanned_aerial_vehicles_amd.trainer import PreTrainedGP
    pre = PreTrainedGP(os.path.join(GOLDEN, "no_such_model.pkl"))
    assert pre.load_dict(reference_pickle_dict(trainer_ref), device=0)
    return pre


def test_pretrained_gp_propagate_horizon(trainer_ref):
    pre = _ref_pre(trainer_ref)
    form = reference_models_form(trainer_ref)
    state, Ug, lin, dt = reference_horizon(trainer_ref)
    N = Ug.shape[1]
    S0, Q = spd(6)
    X, Sig = pre.propagate_horizon(state, Ug, dt, Sigma0=S0, process_noise=Q)
    assert pre._fused_bg, "the six models share inputs and scaler: the one call must have served them"
    assert X.shape == (6, N + 1) and Sig.shape == (N + 1, 6, 6)
    wt, wS, _ = form.run(state[None], np.ascontiguousarray(Ug.T)[None], lin, S0[None], Q)
    check("PreTrainedGP.propagate_horizon: X", X, wt[:, 0].T)
    check("PreTrainedGP.propagate_horizon: Sigma", Sig, wS[:, 0])
    UR = np.stack([Ug, 0.9 * Ug])
    XR, SR = pre.propagate_horizon(state, UR, dt)
    assert XR.shape == (2, 6, N + 1) and SR.shape == (2, N + 1, 6, 6)
    wt, wS, _ = form.run(np.tile(state, (2, 1)), np.ascontiguousarray(UR.transpose(0, 2, 1)), lin)
    check("PreTrainedGP.propagate_horizon, R = 2: X", XR, wt.transpose(1, 2, 0))
    check("PreTrainedGP.propagate_horizon, R = 2: Sigma", SR, wS.transpose(1, 0, 2, 3))


def test_models_that_do_not_share_inputs_take_the_fallback(trainer_ref):
    from unmanned_aerial_vehicles_amd.trainer import StandardScaler
    fused = _ref_pre(trainer_ref)
    pre = _ref_pre(trainer_ref)
    # the same model behind an input scaler of its own (equal numbers, one bit off in one mean): not fusable
    sx = StandardScaler()
    sx.mean_, sx.scale_ = pre.scalers_X["y_residual"].mean_.copy(), pre.scalers_X["y_residual"].scale_.copy()
    sx.mean_[0] = np.nextafter(sx.mean_[0], np.inf)
    pre.scalers_X["y_residual"] = sx
    state, Ug, lin, dt = reference_horizon(trainer_ref)
    S0, Q = spd(6)
    X, Sig = pre.propagate_horizon(state, Ug, dt, Sigma0=S0, process_noise=Q)
    assert pre._fused_bg is False
    wX, wS = fused.propagate_horizon(state, Ug, dt, Sigma0=S0, process_noise=Q)
    assert fused._fused_bg
    check("model by model against the one call: X", X, wX)
    check("model by model against the one call: Sigma", Sig, wS)
    assert Sig[1:].any() and not np.array_equal(X[:, 1], state)


def test_pretrained_gp_propagates_a_file_of_sparse_models(model_dict):
    """A `GPTrainer.sparsify`-style file (six `SparseGP`s behind one input scaler, tests/test_gpu_sparse_batch.py: model_dict) goes
    through `BatchedSparseGP.propagate`; the per-model loop over `predict_residual_jacobian_batch` must agree with it."""
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    from test_gpu_sparse_batch import pretrained
    d, rows = model_dict
    pt, loop_pt = pretrained(d), pretrained(d)
    loop_pt._fused_bg = False
    state, Ug, dt = rows[0, :6], np.ascontiguousarray(rows[:8, 6:].T), 0.02
    S0, Q = spd(6)
    X, Sig = pt.propagate_horizon(state, Ug, dt, Sigma0=S0, process_noise=Q)
    assert isinstance(pt._fused()[0], BatchedSparseGP)
    wX, wS = loop_pt.propagate_horizon(state, Ug, dt, Sigma0=S0, process_noise=Q)
    assert X.shape == (6, 9) and Sig.shape == (9, 6, 6) and np.isfinite(X).all() and np.isfinite(Sig).all()
    check("sparse file, the batch against the per-model loop: X", X, wX)
    check("sparse file, the batch against the per-model loop: Sigma", Sig, wS)
    A = np.eye(6)
    A[0:3, 3:6] = dt * np.eye(3)
    assert not np.allclose(Sig[1], A @ S0 @ A.T + Q, rtol=1e-6, atol=0), "the models' variances must have entered"


# ---- 6. the limits -------------------------------------------------------------------------------------------------------------------
def test_limits():
    from unmanned_aerial_vehicles_amd.batched import BatchedARDGP
    c, bg, _, kw = problem("a")
    lin = c["lin"]
    x1, U1 = rollouts(c["x0"][0], c["U"], 1)
    for what, over in (("coord repeated", dict(coord=(1, 1))), ("coord out of range", dict(coord=(0, 3))),
                       ("in_scale zero", dict(in_scaler=(np.zeros(4), np.array([1.0, 0.0, 1.0, 1.0])))),
                       ("NaN in the input scaler", dict(in_scaler=(np.full(4, np.nan), np.ones(4))))):
        with pytest.raises(ValueError):
            bg.propagate(x1, U1, lin, **dict(kw, **over))
            pytest.fail(what)
    with pytest.raises(ValueError):
        bg.propagate(x1, U1, lin[:1], **kw)                     # nx = 1 < B
    with pytest.raises(RuntimeError):
        BatchedARDGP(optimizer=None).propagate(x1, U1, lin)
    # the entry's own refusals carry the library's message
    sv = bg._serve_state(True, any_dtype=True)
    d0 = sv["dev0"]
    import ctypes as C
    from unmanned_aerial_vehicles_amd import _lib
    from unmanned_aerial_vehicles_amd._lib import host_ptr as hp
    traj, Sigma = np.empty((len(c["U"]) + 1, 1, 3)), np.empty((len(c["U"]) + 1, 1, 3, 3))

    def entry(coord=(0, 1), R=1, H=len(c["U"]), in_scale=None):
        cd = (C.c_int * 2)(*coord)
        return d0.be.call("gpk_propagate_host_multi", 2, sv["X"], sv["alpha"], d0.N, d0.D, hp(sv["ls"]), hp(sv["sf2"]), hp(sv["ym"]),
                          hp(sv["ys"]), sv["W"], d0.Np, d0.Np, hp(sv["kss"]), 0.0, 0, None, 3, cd,
                          None if in_scale is None else hp(np.zeros(4)), None if in_scale is None else hp(in_scale), hp(x1[0]), 1,
                          hp(np.ascontiguousarray(U1[0])), 1, hp(np.ascontiguousarray(lin)), None, 1, None, R, H, hp(traj),
                          hp(Sigma), None, None, None)

    entry()
    for what, msg, over in (("coord repeated", "coord must be distinct", dict(coord=(1, 1))),
                            ("coord out of range", "coord must be in", dict(coord=(0, 3))),
                            ("R = 0", "R must be in", dict(R=0)), ("H = 257", "H must be in", dict(H=257)),
                            ("in_scale zero", "in_scale must be non-zero", dict(in_scale=np.array([1.0, 0.0, 1.0, 1.0])))):
        with pytest.raises(_lib.GPKError, match=msg) as ei:
            entry(**over)
            pytest.fail(what)
        assert ei.value.code == _lib.GPK_BAD_ARG
    check("after the refusals", bg.propagate(x1, U1, lin, **kw)[0], problem("a")[2].run(x1, U1, lin)[0])
