"""Exact moment matching of the per-axis batch (DESIGN.md, K11 "moment matching") on the GPU: `BatchedARDGP.predict_moments` (one C
call, `gpk_moments_host_multi`: all B (B + 1) / 2 pairs of models) and `propagate(method="moment")`
(`gpk_propagate_mm_host_multi`), its host route and `PreTrainedGP.propagate_horizon`, in raw units.  Buffers start out as NaN
(conftest: GPK_DEBUG_FILL).

Expected values: `moments_numpy_form` of tests/test_moments_host.py on the dense NumPy posteriors of tests/test_propagate_host.py,
with the input scaler, the output scaler and the coordinate map around them.  Bar: the project's fp64 bar, 1e-8 of each array's
largest component.  Bit identity is asserted with np.array_equal.

Inputs: tests/golden/axis_paths_ref.npz, cases (N, D, B, nx, H) = a (120, 4, 2, 3, 6), csv (200, 10, 6, 6, 25), gap (96, 10, 4, 6,
5; coord = (0, 2, 3, 5): a non-default coordinate map with free coordinates), one (128, 3, 1, 2, 4), and csv's models 3..5 alone on
coord = (3, 4, 5)."""
import numpy as np
import pytest

from test_gpu_axis_propagate import problem
from test_gpu_moments import check_moments, check_run
from test_gpu_paths import check
from test_moments_host import moments_numpy_form
from test_propagate_host import rollouts, spd

pytestmark = pytest.mark.gpu

_forms = {}


def setup(name):
    """(arrays, batch, moments form, coord, keyword arguments of `propagate`) of a case: the form built once"""
    c, bg, form, kw = problem(name)
    if name not in _forms:
        _forms[name] = moments_numpy_form(form.gps, form.in_scaler, form.out)
    return c, bg, _forms[name], list(kw["coord"]), kw


# ---- 1. parity with the NumPy form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R", [("a", 1), ("a", 5), ("a", 17), ("a", 32), ("gap", 1), ("gap", 5), ("gap", 17), ("gap", 32),
                                    ("one", 5), ("one", 32), ("csv", 5), ("csv345", 17), ("csv345", 32)])
def test_predict_moments_parity(name, R):
    c, bg, mform, _, kw = setup(name)
    nx, B = c["lin"].shape[0], len(bg.models)
    S0, _ = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"], R)
    Q = np.ascontiguousarray(np.concatenate([x0, U[:, 0]], axis=1))
    S = np.stack([S0 * (0.05 + 0.01 * r) for r in range(R)])
    sc = dict(in_scaler=kw["in_scaler"], out_scaler=kw["out_scaler"])
    for noisy in (False, True):
        got = bg.predict_moments(Q, S, var_includes_noise=noisy, **sc)
        assert got[0].shape == (R, B) and got[1].shape == (R, B, B) and got[2].shape == (R, B, Q.shape[1])
        check_moments(f"batch {name}, R = {R}, noise {noisy}", got, mform.batch(Q, S, noisy))
        assert np.array_equal(got[1], got[1].transpose(0, 2, 1)), "every V block equals its transpose bit for bit"
    # without the scalers: the models' own units
    plain = moments_numpy_form(mform.gps)
    check_moments(f"batch {name}, R = {R}, no scalers", bg.predict_moments(Q, S), plain.batch(Q, S, False))


@pytest.mark.parametrize("name", ("a", "csv", "csv345", "gap", "one"))
def test_propagate_parity(name):
    c, bg, mform, coord, kw = setup(name)
    lin = c["lin"]
    nx, H, B = lin.shape[0], len(c["U"]), len(bg.models)
    S0, Q = spd(nx)
    S0 = 0.05 * S0
    for R in ((1, 5) if name == "csv" else (1, 5, 17, 32)):
        # (the whole horizon at R = 1 and 5; its first four stages at 17 and 32, where the NumPy form is what takes the time)
        Uc = c["U"] if R <= 5 else c["U"][:4]
        H = len(Uc)
        x0, U = rollouts(c["x0"][0], Uc, R)
        if R == 1 or (name != "csv" and R == 5):
            for noisy in (False, True):
                got = bg.propagate(x0, U, lin, var_includes_noise=noisy, return_stages=True, method="moment", **kw)
                assert got[0].shape == (H + 1, R, nx) and got[2]["cov"].shape == (H, R, B, B)
                assert np.array_equal(got[0][0], x0) and not got[1][0].any()
                check_run(f"batch {name}, R = {R}, noise {noisy}, Sigma0 = 0", got, mform.run(coord, x0, U, lin, None, None, noisy))
        got = bg.propagate(x0, U, lin, Sigma0=S0, process_noise=Q, return_stages=True, method="moment", **kw)
        check_run(f"batch {name}, R = {R}, SPD Sigma0 and Q", got, mform.run(coord, x0, U, lin, np.tile(S0, (R, 1, 1)), Q))
        assert np.array_equal(got[1], got[1].transpose(0, 1, 3, 2)), "every Sigma[h, r] equals its transpose bit for bit"
        assert np.array_equal(got[2]["cov"], got[2]["cov"].transpose(0, 1, 3, 2))
    # a coordinate without a model advances by lin alone; its variance is the propagated one alone
    free = [i for i in range(nx) if i not in coord]
    if free:
        traj, Sigma = bg.propagate(c["x0"][0], c["U"], lin, method="moment", **kw)
        q0 = np.concatenate([c["x0"][0], c["U"][0]])
        assert np.allclose(traj[1, 0, free], (c["x0"][0] + lin @ q0)[free], rtol=1e-14, atol=0)
        assert not Sigma[1, 0][free][:, free].any()


# ---- 2. independent device checks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("a", "gap"))
def test_zero_covariance_is_the_linear_stage_and_predict(name):
    c, bg, _, coord, kw = setup(name)
    lin = c["lin"]
    nx = lin.shape[0]
    x0, U = rollouts(c["x0"][0], c["U"][:1], 5)
    _, Q = spd(nx)
    lt, lS, ls = bg.propagate(x0, U, lin, process_noise=Q, return_stages=True, **kw)
    mt, mS, ms = bg.propagate(x0, U, lin, process_noise=Q, return_stages=True, method="moment", **kw)
    check(f"batch {name}: H = 1, Sigma0 = 0, traj against the linear chain", mt, lt)
    check(f"batch {name}: H = 1, Sigma0 = 0, Sigma against the linear chain", mS, lS)
    check(f"batch {name}: mean at Sigma = 0 against the linear stage", ms["mean"], ls["mean"])
    B = len(bg.models)
    check(f"batch {name}: variance at Sigma = 0 against the linear stage", ms["cov"][:, :, np.arange(B), np.arange(B)], ls["var"])
    assert not ms["xcov"].any()


@pytest.mark.parametrize("name", ("a", "gap"))
def test_host_route_and_stage_bits(name):
    c, bg, _, coord, kw = setup(name)
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"][:4], 17)
    args = dict(Sigma0=0.05 * S0, process_noise=Q, return_stages=True, method="moment", **kw)
    chain, host = bg.propagate(x0, U, lin, **args), bg.propagate(x0, U, lin, route="host", **args)
    check_run(f"batch {name}: the host route against the chain", host, chain)
    traj, Sigma, st = chain
    for h in range(U.shape[1]):
        q = np.ascontiguousarray(np.concatenate([traj[h], U[:, h]], axis=1))
        mean, cov, xcov = bg.predict_moments(q, Sigma[h], in_scaler=kw["in_scaler"], out_scaler=kw["out_scaler"])
        assert np.array_equal(st["mean"][h], mean), (name, h, "mean")
        assert np.array_equal(st["cov"][h], cov), (name, h, "cov")
        assert np.array_equal(st["xcov"][h], xcov), (name, h, "xcov")


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------
def test_repeatable_and_independent_of_the_batch():
    c, bg, _, coord, kw = setup("gap")
    lin = c["lin"]
    S0, Q = spd(lin.shape[0])
    x0, U = rollouts(c["x0"][0], c["U"], 17)
    args = dict(Sigma0=0.05 * S0, process_noise=Q, return_stages=True, method="moment", **kw)
    one, two = bg.propagate(x0, U, lin, **args), bg.propagate(x0, U, lin, **args)
    for a, b in zip(one[:2] + tuple(one[2].values()), two[:2] + tuple(two[2].values())):
        assert np.array_equal(a, b), "two calls return the same bits"
    for r in (0, 16):
        alone = bg.propagate(x0[r], U[r], lin, **args)
        assert np.array_equal(alone[0][:, 0], one[0][:, r]) and np.array_equal(alone[1][:, 0], one[1][:, r]), r


def test_a_column_has_the_bits_of_the_model_served_alone():
    from unmanned_aerial_vehicles_amd import BatchedARDGP
    c, bg, _, _, kw = setup("a")
    nx = c["lin"].shape[0]
    S0, _ = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    Q = np.ascontiguousarray(np.concatenate([x0, U[:, 0]], axis=1))
    mean, cov, xcov = bg.predict_moments(Q, 0.05 * S0, in_scaler=kw["in_scaler"], out_scaler=kw["out_scaler"])
    for b, m in enumerate(bg.models):
        solo = BatchedARDGP(optimizer=None)
        solo.models = [m]
        out = (kw["out_scaler"][0][b:b + 1], kw["out_scaler"][1][b:b + 1])
        m1, c1, x1 = solo.predict_moments(Q, 0.05 * S0, in_scaler=kw["in_scaler"], out_scaler=out)
        assert np.array_equal(m1[:, 0], mean[:, b]) and np.array_equal(c1[:, 0, 0], cov[:, b, b]), b
        assert np.array_equal(x1[:, 0], xcov[:, b]), b


def test_linear_is_untouched():
    c, bg, _, _, kw = setup("a")
    S0, Q = spd(c["lin"].shape[0])
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    a = bg.propagate(x0, U, c["lin"], Sigma0=S0, process_noise=Q, return_stages=True, **kw)
    b = bg.propagate(x0, U, c["lin"], Sigma0=S0, process_noise=Q, return_stages=True, method="linear", **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(a[2][k], b[2][k]) for k in ("mean", "var", "jac"))


# ---- 4. refusals and the wrapper -------------------------------------------------------------------------------------------------
def test_refusals():
    from unmanned_aerial_vehicles_amd.sparse_batch import BatchedSparseGP
    c, bg, _, _, kw = setup("a")
    x0, U = rollouts(c["x0"][0], c["U"], 33)
    with pytest.raises(ValueError, match="R must be"):
        bg.propagate(x0, U, c["lin"], method="moment", **kw)
    with pytest.raises(ValueError, match="order=1"):
        bg.propagate(x0[:2], U[:2], c["lin"], method="moment", order=2, **kw)
    with pytest.raises(ValueError, match="propagate_gradient"):
        bg.propagate_gradient(x0[:1], U[:1], c["lin"], np.zeros((len(c["U"]) + 1, 1, c["lin"].shape[0])), method="moment", **kw)
    with pytest.raises(ValueError, match="BatchedSparseGP"):
        BatchedSparseGP.propagate(BatchedSparseGP.__new__(BatchedSparseGP), x0[:1], U[:1], c["lin"], method="moment")


def test_pretrained_wrapper(trainer_ref, capsys):
    from test_gpu_axis_propagate import _ref_pre
    from test_propagate_host import reference_horizon, reference_models_form
    pre = _ref_pre(trainer_ref)
    form = reference_models_form(trainer_ref)
    state, Ug, lin, dt = reference_horizon(trainer_ref)
    S0, Q = spd(6)
    X, Sig = pre.propagate_horizon(state, Ug, dt, Sigma0=1e-3 * S0, process_noise=1e-2 * Q, method="moment")
    assert "failed" not in capsys.readouterr().out
    mform = moments_numpy_form(form.gps, form.in_scaler, form.out)
    wt, wS, _ = mform.run(range(6), state[None], np.ascontiguousarray(Ug[:4].T)[None], lin, 1e-3 * S0[None], 1e-2 * Q)
    check("PreTrainedGP.propagate_horizon(method='moment'): X", X, wt[:, 0].T)
    check("PreTrainedGP.propagate_horizon(method='moment'): Sigma", Sig, wS[:, 0])
    X, Sig = pre.propagate_horizon(state, Ug, dt, Sigma0=np.full((6, 6), np.inf), method="moment")
    assert "failed" in capsys.readouterr().out and np.isfinite(Sig).all()
    with pytest.raises(ValueError, match="order=1"):
        pre.propagate_horizon(state, Ug, dt, method="moment", order=2)
