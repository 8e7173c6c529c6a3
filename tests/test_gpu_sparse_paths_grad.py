"""Path gradients ("path gradients") on the GPU, the sparse models: `SparsePosteriorPaths` and
`BatchedSparsePosteriorPaths` `.step` / `.rollout` with return_jacobian=True (the batch through the _z entries: own Z per model),
`SimpleQuadrotorGP.sample_rollouts` with a `SparseGP` and `PreTrainedGP.sample_rollouts` on sparse models.  Buffers start out as
NaN (conftest: GPK_DEBUG_FILL).

Expected values: the closed form in NumPy (tests/test_gpu_paths_grad.py) on the fixture module's dense forms.  Bar: the fp64 bar,
1e-8 of each array's largest component; bits with tobytes() / np.array_equal.  Cases: those of tests/test_gpu_sparse_paths.py."""
import numpy as np
import pytest

from test_gpu_paths import check
from test_gpu_paths_grad import (FD_BAR, axis_jac_numpy_form, axis_rollout_jac_numpy_form, central_differences, input_scale,
                                 jac_numpy_form, jshape, rollout_jac_numpy_form)
from test_gpu_sparse_paths import BATCH, ROLLOUT_BATCH, SINGLE, G, case, double_integrator, load_case, sparse_model, trainer_dict

pytestmark = pytest.mark.gpu


def roll(paths, c, jac=True, **over):
    a = dict(x0=c["x0"], U=c["U"], lin=c["lin"], coord=c["coord"], in_scaler=(c["in"][0], c["in"][1]))
    a.update(over)
    return paths.rollout(a["x0"], a["U"], a["lin"], coord=a["coord"], in_scaler=a["in_scaler"], return_jacobian=jac)


# ---- 1. parity, value bits, repeatability ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE)
def test_single_model_parity_value_bits_and_repeatability(name):
    c, sp, paths, form = case(name)
    S, P, D, H = c["weights"].shape[1], c["weights"].shape[2], c["Z"].shape[1], len(c["U"])
    val, jac = paths.step(c["Xs"], return_jacobian=True)
    assert jac.shape == ((S, D) if P == 1 else (S, P, D))
    check(f"case {name}: step jac", jac, jshape(jac_numpy_form(form, c["Xs"]), P))
    assert val.tobytes() == paths.step(c["Xs"]).tobytes(), "the value keeps its bits"
    assert paths.step(c["Xs"], return_jacobian=True)[1].tobytes() == jac.tobytes(), "the same bits every call"
    traj, rj = paths.rollout(c["x0"], c["U"], c["lin"], return_jacobian=True)
    assert traj.shape == (H + 1, S, P) and rj.shape == (H, S, P, D)
    assert traj.tobytes() == paths.rollout(c["x0"], c["U"], c["lin"]).tobytes(), "the trajectory keeps its bits"
    check(f"case {name}: rollout jac", rj, rollout_jac_numpy_form(form, form.rollout(c["x0"], c["U"], c["lin"]), c["U"]))
    assert paths.rollout(c["x0"], c["U"], c["lin"], return_jacobian=True)[1].tobytes() == rj.tobytes(), "the same bits every call"


@pytest.mark.parametrize("name", BATCH)
def test_batch_parity_value_bits_and_repeatability(name):
    c, bg, paths, form = case(name)
    B, S, D = c["weights"].shape[0], c["weights"].shape[2], c["Z"].shape[2]
    val, jac = paths.step(c["Xs"], return_jacobian=True)
    assert jac.shape == (S, B, D)
    check(f"case {name}: step jac", jac, axis_jac_numpy_form(form, c["Xs"]))
    assert val.tobytes() == paths.step(c["Xs"]).tobytes(), "the value keeps its bits"
    assert paths.step(c["Xs"], return_jacobian=True)[1].tobytes() == jac.tobytes(), "the same bits every call"
    if name in ROLLOUT_BATCH:
        traj, rj = roll(paths, c)
        assert traj.shape == c["traj"].shape and rj.shape == (len(c["U"]), S, B, D)
        assert traj.tobytes() == roll(paths, c, jac=False).tobytes(), "the trajectory keeps its bits"
        sc = (c["in"][0], c["in"][1])
        check(f"case {name}: rollout jac", rj,
              axis_rollout_jac_numpy_form(form, form.rollout(c["x0"], c["U"], c["lin"], c["coord"], sc), c["U"], sc))
        assert roll(paths, c)[1].tobytes() == rj.tobytes(), "the same bits every call"
    coef = paths.coef.cpu().numpy()
    assert paths.mstride > S and np.isnan(coef.reshape(len(coef), B, paths.mstride)[:, :, S:]).all(), "the padding between the blocks"


# ---- 2. the bits of the single-model gradient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c", "e", "f"))
def test_every_column_has_the_bits_of_its_own_single_model_jacobian(name):
    from unmanned_aerial_vehicles_amd import BatchedSparsePosteriorPaths, SparsePosteriorPaths
    c, bg, _, _ = case(name)
    B = c["weights"].shape[0]
    batch = BatchedSparsePosteriorPaths.from_randomness(bg, c["omega"], c["phase"], c["weights"], c["xi"])       # no output scaler
    val, jac = batch.step(c["Xs"], return_jacobian=True)
    assert np.isfinite(jac).all()
    for b in range(B):
        single = SparsePosteriorPaths.from_randomness(bg.models[b], c["omega"][b], c["phase"][b], c["weights"][b], c["xi"][b])
        sv, sj = single.step(c["Xs"], return_jacobian=True)
        assert np.array_equal(val[:, b], sv), f"case {name}: column {b} of the value"
        assert np.array_equal(jac[:, b], sj), f"case {name}: column {b} of jac"


# ---- 3. anchors against code that exists -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE + BATCH)
def test_zero_randomness_is_the_sparse_mean_jacobian(name):
    from unmanned_aerial_vehicles_amd import BatchedSparsePosteriorPaths, SparsePosteriorPaths
    c, model, _, _ = case(name)
    cls = SparsePosteriorPaths if name in SINGLE else BatchedSparsePosteriorPaths
    zero = cls.from_randomness(model, c["omega"], c["phase"], np.zeros_like(c["weights"]), np.zeros_like(c["xi"]))
    Q = np.resize(c["Xq"], (zero.S, zero.D))
    check(f"case {name}: step jac with xi = 0, w = 0 against predict_jacobian", zero.step(Q, return_jacobian=True)[1],
          np.asarray(model.predict_jacobian(Q)[1]))


@pytest.mark.parametrize("name", SINGLE + ROLLOUT_BATCH)
def test_one_stage_rollout_is_the_step_jacobian(name):
    c, _, paths, _ = case(name)
    S = c["x0"].shape[0]
    q = np.concatenate([c["x0"], np.broadcast_to(c["U"][0], (S, len(c["U"][0])))], axis=1)
    if name in SINGLE:
        want = paths.step(q, return_jacobian=True)[1].reshape(S, paths.P, paths.D)
        got = paths.rollout(c["x0"], c["U"][:1], c["lin"], return_jacobian=True)[1]
    else:
        shift, scale = c["in"]
        want = paths.step((q - shift) / scale, return_jacobian=True)[1] / scale
        got = roll(paths, c, U=c["U"][:1])[1]
    check(f"case {name}: jac[0] of a one-stage rollout against the step Jacobian", got[0], want)


@pytest.mark.parametrize("name", SINGLE + BATCH)
def test_step_jacobian_agrees_with_central_differences_of_step(name):
    c, _, paths, _ = case(name)
    Zall = c["Z"].reshape(-1, c["Z"].shape[-1])
    jac = paths.step(c["Xs"], return_jacobian=True)[1]
    fd = central_differences(paths.step, c["Xs"], input_scale(Zall))
    check(f"case {name}: step jac against central differences of step on the device", jac, fd.reshape(jac.shape), FD_BAR)


# ---- 4. the two sample_rollouts --------------------------------------------------------------------------------------------------------
def test_simple_quadrotor_gp_sample_rollouts_with_a_sparse_model_and_jacobian(capsys):
    from unmanned_aerial_vehicles_amd import SimpleQuadrotorGP, draw_sparse_path_randomness
    c = load_case("c")
    dt, R, F, H = 0.02, 5, 32, 25
    hyper, ym, ys = c["hyper"][0], c["ynorm"][0], c["ynorm"][1]
    sp = sparse_model(c["Z"][0], c["X"], c["Y"], c["ls"][0], hyper, ym, ys)
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = sp, True
    state, U_guess = 0.3 * c["Xq"][0, :6], 0.3 * c["Xq"][:4, 6:].T @ np.ones((4, H)) / 4.0 + 0.1 * np.sin(np.arange(H))[None]
    lin = double_integrator(dt)
    X, J = sq.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7, return_jacobian=True)
    assert X.shape == (R, 6, H + 1) and J.shape == (R, H, 6, 10)
    assert X.tobytes() == sq.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7).tobytes()
    r = draw_sparse_path_randomness(np.random.RandomState(7), 64, 10, F, R, 6, c["ls"][0])
    form = G.SparseForm(c["Z"][0], c["X"], c["Y"], c["ls"][0], *hyper, ym, ys, r["omega"], r["phase"], r["weights"], r["xi"])
    check("sample_rollouts with a SparseGP: J against the NumPy form", J,
          rollout_jac_numpy_form(form, form.rollout(state, U_guess.T, lin), U_guess.T).transpose(1, 0, 2, 3))
    capsys.readouterr()
    bad, J0 = sq.sample_rollouts(state, np.full((4, H), np.nan), dt, n_rollouts=R, n_features=F, random_state=7, return_jacobian=True)
    assert bad.shape == (R, 6, H + 1) and J0.shape == (R, H, 6, 10) and not J0.any()
    assert "GP rollout sampling failed" in capsys.readouterr().out


def test_pretrained_gp_sample_rollouts_on_sparse_models_with_jacobian(capsys):
    from unmanned_aerial_vehicles_amd import PreTrainedGP, draw_sparse_batch_path_randomness
    c = load_case("c")
    dt, R, F, H = 0.02, 5, 32, 25
    models = [sparse_model(c["Z"][b], c["X"], c["Y"][:, b:b + 1], c["ls"][b], c["hyper"][b], c["ynorm"][0, b:b + 1],
                           c["ynorm"][1, b:b + 1]) for b in range(6)]
    state, U_guess = c["x0"][0], c["U"].T
    pg = PreTrainedGP("/nonexistent/model.pkl")
    keep = [0, 2, 3, 4, 5]
    assert pg.load_dict(trainer_dict(c, models, keep))
    capsys.readouterr()
    X, J = pg.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7, return_jacobian=True)
    assert "failed" not in capsys.readouterr().out
    assert X.shape == (R, 6, H + 1) and J.shape == (R, H, 6, 10)
    assert X.tobytes() == pg.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7).tobytes()
    r = draw_sparse_batch_path_randomness(np.random.RandomState(7), 64, 10, F, R, c["ls"][keep])
    form = G.SparseBatchForm(c["Z"][keep], c["X"], c["Y"][:, keep], c["ls"][keep], c["hyper"][keep], c["ynorm"][:, keep], r["omega"],
                             r["phase"], r["weights"], r["xi"], (c["out"][0][keep], c["out"][1][keep]))
    sc = (c["in"][0], c["in"][1])
    want = np.zeros((R, H, 6, 10))
    want[:, :, keep] = axis_rollout_jac_numpy_form(form, form.rollout(state, c["U"], c["lin"], keep, sc), c["U"], sc).transpose(1, 0, 2, 3)
    check("sample_rollouts on sparse models: J against the NumPy form", J, want)
    assert not J[:, :, 1].any(), "a coordinate without a model has a zero row"
    bad, J0 = pg.sample_rollouts(state, np.full((4, H), np.nan), dt, n_rollouts=R, n_features=F, random_state=7, return_jacobian=True)
    assert bad.shape == (R, 6, H + 1) and J0.shape == (R, H, 6, 10) and not J0.any()
    assert "GP rollout sampling failed" in capsys.readouterr().out


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_wrong_shapes_and_non_finite_inputs_raise_value_errors():
    for name in ("a", "d"):
        c, _, paths, form = case(name)
        Xs, x0, U, lin = c["Xs"], c["x0"], c["U"], c["lin"]
        for bad in (Xs[:, :2], np.concatenate([Xs, Xs]), np.full_like(Xs, np.nan), np.full_like(Xs, np.inf)):
            with pytest.raises(ValueError):
                paths.step(bad, return_jacobian=True)
        for bad in ((np.concatenate([x0, x0]), U, lin), (x0, U[:, :0], lin), (x0, U, lin[:, :2]), (x0, np.zeros((257, U.shape[1])), lin),
                    (np.full_like(x0, np.nan), U, lin), (x0, np.full_like(U, np.inf), lin)):
            with pytest.raises(ValueError):
                paths.rollout(*bad, return_jacobian=True)
        want = jshape(jac_numpy_form(form, Xs), paths.P) if name == "a" else axis_jac_numpy_form(form, Xs)
        check(f"case {name}: step jac after the refusals", paths.step(Xs, return_jacobian=True)[1], want)
