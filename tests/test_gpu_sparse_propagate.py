"""Horizon propagation on the sparse posteriors as ONE C call ("the sparse chain") on the GPU:
`SparseGP.propagate(route="chain")` (`gpk_sparse_propagate`), `BatchedSparseGP.propagate(route="chain")`
(`gpk_sparse_propagate_multi`) and the control-loop wrappers on top of them.  Buffers start out as NaN (conftest:
GPK_DEBUG_FILL), so a stage that read query padding, a padded row of a factor or an unwritten share would show.

Expected values: `propagate_numpy_form` (tests/test_propagate_host.py) on the dense form of the sparse posteriors.  Bar: the
project's fp64 bar, 1e-8 of each array's largest component.  What it rests on is printed and asserted by
tests/test_sparse_propagate_host.py, which also defines the problems: on every horizon here the latent variance stays above 2.5 %
of the prior - the chain's clip (1e-10, normalised units) and the host loop's (0) are never active, so the two latent variances
differ in rounding only - and a 1e-12 perturbation of x0 grows about 2x at most.  Bit identity is asserted with np.array_equal.

Shapes: m = 26 (single3), 60 (batch2, batch8) -> mp = 128, eight variance workgroups per factor with padded rows; m = 200
(one200) -> mp = 256; D = 10 (4 for single3), H = 5; R = 1, 5 for parity and 1, 16, 17, 32 for the bits (both 16-query column
block counts, both sides of the 16-row edge)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_paths import check
from test_gpu_propagate import check_all
from test_gpu_sparse_batch import model_dict  # noqa: F401  (the fixture: six sparse models behind one input scaler)
from test_propagate_host import rollouts, spd
from test_sparse_propagate_host import PROBLEMS, problem

pytestmark = pytest.mark.gpu

_models = {}


def served(name):
    """the object that serves a problem - a `SparseGP` (single3, one200) or a `BatchedSparseGP`: built once, shared, left unchanged"""
    if name not in _models:
        from unmanned_aerial_vehicles_amd import RBF, BatchedSparseGP, ConstantKernel, SparseGP, WhiteKernel
        from test_gpu_sparse_batch import build_model, case
        c = problem(name)[0]
        if name == "single3":
            sf2, noise, alpha = c["hyper"]
            _models[name] = SparseGP(ConstantKernel(sf2) * RBF(c["ls"]) + WhiteKernel(noise), c["Z"], alpha=alpha,
                                     y_mean=c["Y"].mean(axis=0), y_std=c["Y"].std(axis=0)).fit(c["X"], c["Y"])
        elif name == "batch2":
            _models[name] = case(2, 60, 400, 10)[2]
        elif name == "batch8":
            _models[name] = BatchedSparseGP([build_model(p) for p in c["ps"]])
        else:
            _models[name] = build_model(c["ps"][0])
    return _models[name]


def same_bits(tag, a, b):
    assert np.array_equal(a[0], b[0]), f"{tag}: traj"
    assert np.array_equal(a[1], b[1]), f"{tag}: Sigma"
    if len(a) > 2:
        for k in ("mean", "var", "jac"):
            assert np.array_equal(a[2][k], b[2][k]), f"{tag}: {k}"


def worst(a, b):
    """the largest difference of two results, each array relative to its largest component"""
    pairs = [(a[0], b[0]), (a[1], b[1])] + [(a[2][k], b[2][k]) for k in ("mean", "var", "jac")]
    return max(float(np.max(np.abs(x - y)) / np.max(np.abs(y))) for x, y in pairs)


# ---- 1. parity with the NumPy form, and with the host loop ---------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_parity_with_the_numpy_form_and_the_host_loop(name):
    c, form, kw, _ = problem(name)
    gp = served(name)
    assert gp.propagate_ok()
    lin = c["lin"]
    nx, D = lin.shape
    NO = form.NO
    S0, Q = spd(nx)
    for R in (1, 5):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        H = U.shape[1]
        for noisy in (False, True):
            for tag, extra, want_args in (("Sigma0 = 0", {}, (None, None)),
                                          ("SPD Sigma0 and Q", dict(Sigma0=S0, process_noise=Q), (np.tile(S0, (R, 1, 1)), Q))):
                args = dict(var_includes_noise=noisy, return_stages=True, **kw, **extra)
                got = gp.propagate(x0, U, lin, route="chain", **args)
                assert got[0].shape == (H + 1, R, nx) and got[1].shape == (H + 1, R, nx, nx)
                assert got[2]["mean"].shape == (H, R, NO) and got[2]["jac"].shape == (H, R, NO, D)
                assert np.array_equal(got[0][0], x0)
                check_all(f"{name}, R = {R}, noise {noisy}, {tag}", got, form.run(x0, U, lin, *want_args, noisy=noisy))
                loop = gp.propagate(x0, U, lin, route="host", **args)
                print(f"{name}, R = {R}, noise {noisy}, {tag}: chain against the host loop, largest difference {worst(got, loop):.2e}")
                check_all(f"{name}, R = {R}, noise {noisy}, {tag}, against route = host", got, loop)
    # the shorthand shapes, two results without return_stages; "auto" is still the host loop, bit for bit
    one = gp.propagate(c["x0"][0], c["U"], lin, route="chain", **kw)
    assert len(one) == 2 and one[0].shape == (len(c["U"]) + 1, 1, nx)
    same_bits(f"{name}: auto is the host loop", gp.propagate(c["x0"][0], c["U"], lin, **kw),
              gp.propagate(c["x0"][0], c["U"], lin, route="host", **kw))


# ---- 2. the stage outputs have the bits of predict_jacobian at the returned rows ------------------------------------------------
@pytest.mark.parametrize("R", (1, 16, 17, 32))
@pytest.mark.parametrize("name", ("single3", "batch2"))
def test_stage_outputs_have_the_bits_of_predict_jacobian(name, R):
    c = problem(name)[0]
    gp = served(name)
    x0, U = rollouts(c["x0"][0], c["U"], R)
    kw = {} if name == "single3" else dict(coord=c["coord"])
    traj, Sigma, st = gp.propagate(x0, U, c["lin"], var_includes_noise=True, return_stages=True, route="chain", **kw)
    for h in range(U.shape[1]):
        q = np.ascontiguousarray(np.concatenate([traj[h], U[:, h]], axis=1))
        mean, dmean, var, _ = gp.predict_jacobian(q, return_var=True)
        assert np.array_equal(st["mean"][h], mean), (name, R, h, "mean")
        assert np.array_equal(st["jac"][h], dmean), (name, R, h, "jac")
        assert np.array_equal(st["var"][h], var), (name, R, h, "var")


# ---- 3. batch bits ---------------------------------------------------------------------------------------------------------------------
def test_one_model_batch_has_the_bits_of_the_single_model_chain():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    c = problem("one200")[0]
    gp = served("one200")
    bg = BatchedSparseGP([gp])
    S0, Q = spd(1)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    for noisy in (False, True):
        args = dict(Sigma0=S0, process_noise=Q, var_includes_noise=noisy, return_stages=True, route="chain")
        same_bits(f"B = 1 against the model's own chain, noise {noisy}", bg.propagate(x0, U, c["lin"], **args),
                  gp.propagate(x0, U, c["lin"], **args))


def test_column_b_of_three_models_has_the_bits_of_model_b_at_stage_0():
    """A model's own chain has its one output as its whole state, so along a horizon its queries cannot follow the batch's
    (the other models' coordinates would have to be its controls, and they move with those models).  At stage 0 the queries can
    be made to coincide: there column b of the batch's stage outputs must be model b's own, bit for bit."""
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    models = served("batch8").models[:3]
    bg = BatchedSparseGP(models)
    rng = np.random.default_rng(33)
    lin3 = 0.05 * rng.standard_normal((3, 10))
    for R in (1, 17):
        x0 = 0.4 * rng.standard_normal((R, 3))
        U = 0.4 * rng.standard_normal((R, 2, 7))
        st = bg.propagate(x0, U, lin3, var_includes_noise=True, return_stages=True, route="chain")[2]
        q0 = np.concatenate([x0, U[:, 0]], axis=1)
        for b, gp in enumerate(models):
            own = gp.propagate(np.ascontiguousarray(q0[:, :1]), np.ascontiguousarray(q0[:, None, 1:]), lin3[:1],
                               var_includes_noise=True, return_stages=True, route="chain")[2]
            for k in ("mean", "var", "jac"):
                assert np.array_equal(st[k][0][:, b], own[k][0][:, 0]), (R, b, k)


# ---- 4. Sigma: symmetric, positive semi-definite, diag(var) after one stage; the same bits every call -----------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_sigma_properties_and_repeatability(name):
    c, form, kw, _ = problem(name)
    gp = served(name)
    nx = c["lin"].shape[0]
    S0, Q = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    for extra in ({}, {"Sigma0": S0, "process_noise": Q}):
        a = gp.propagate(x0, U, c["lin"], return_stages=True, route="chain", **kw, **extra)
        b = gp.propagate(x0, U, c["lin"], return_stages=True, route="chain", **kw, **extra)
        same_bits(f"{name}: two calls", a, b)
        Sigma = a[1]
        assert np.array_equal(Sigma, Sigma.transpose(0, 1, 3, 2)), "every Sigma[h, r] equals its transpose bit for bit"
        ev = np.linalg.eigvalsh(Sigma)[..., 0]
        tr = np.trace(Sigma, axis1=2, axis2=3)
        print(f"{name}: smallest eigenvalue + 1e-12 trace, worst over the horizon: {float(np.min(ev + 1e-12 * tr)):.3e}")
        assert (ev >= -1e-12 * tr).all()
        if not extra:
            want = np.zeros((5, nx, nx))
            want[:, form.coord, form.coord] = a[2]["var"][0]
            assert np.array_equal(Sigma[1], want), "Sigma_1 = diag(var) on the driven coordinates, bit for bit"


# ---- 5. an independent device route: the rollout of a path set without randomness ------------------------------------------------
def test_traj_equals_the_rollout_of_a_zero_randomness_path_set():
    """With zero weights and zero xi a sparse path is k_u(x)^T Kuu^-1 m_u, the posterior mean through another kernel chain."""
    from unmanned_aerial_vehicles_amd.paths import SparsePosteriorPaths
    c = problem("single3")[0]
    gp = served("single3")
    R, F = 4, 16
    m, D = c["Z"].shape
    rng = np.random.default_rng(5)
    zero = SparsePosteriorPaths.from_randomness(gp, rng.standard_normal((F, D)) / c["ls"], rng.uniform(0, 2 * np.pi, F),
                                                np.zeros((F, R, 3)), np.zeros((m, R, 3)))
    x0, _ = rollouts(c["x0"][0], c["U"], R)
    want = zero.rollout(x0, c["U"], c["lin"])
    check("single3: traj against the mean path's rollout", gp.propagate(x0, c["U"], c["lin"], route="chain")[0], want)


# ---- 6. the limits: refusals, and the same bits afterwards -----------------------------------------------------------------------
def test_limits_are_refused_and_leave_the_handle_serving():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP, _lib
    from unmanned_aerial_vehicles_amd._lib import host_ptr as hp
    from test_gpu_sparse_batch import build_model, model_inputs
    c, _, kw, _ = problem("batch2")
    bg = served("batch2")
    lin = c["lin"]
    x1, U1 = rollouts(c["x0"][0], c["U"], 1)
    first = bg.propagate(x1, U1, lin, return_stages=True, route="chain", **kw)
    # the Python side: argument checks before any device call
    x33, U33 = rollouts(c["x0"][0], c["U"], 33)
    for what, args, over in (("R = 33", (x33, U33, lin), {}), ("H = 257", (x1, np.zeros((1, 257, 4)), lin), {}),
                             ("nx > D", (np.zeros(11), np.zeros((5, 0)), np.zeros((11, 10))), {}),
                             ("nx < B", (x1[:, :1], np.zeros((1, 5, 9)), lin[:1]), {}),
                             ("coord repeated", (x1, U1, lin), dict(coord=(1, 1))),
                             ("in_scale zero", (x1, U1, lin), dict(in_scaler=(np.zeros(10), np.zeros(10)))),
                             ("an unknown route", (x1, U1, lin), dict(route="device"))):
        with pytest.raises(ValueError):
            bg.propagate(*args, **dict(dict(kw, route="chain"), **over))
            pytest.fail(what)
    # the entry's own refusals: GPK_BAD_ARG with the library's message
    other = build_model(model_inputs(0, 61, 400, 10))      # another m
    raw = build_model(model_inputs(1, 60, 400, 10))        # rows, but never finalised
    other._ensure()
    bes, good = bg._ensure()
    be = bes[0]
    traj, Sigma = np.empty((6, 1, 6)), np.empty((6, 1, 6, 6))
    cd = (C.c_int * 2)(*c["coord"])

    def handles(*gps):
        return (C.c_void_p * len(gps))(*[g._backend().h.value for g in gps])

    def entry(hs=good, B=2, nx=6, R=1, H=5, coord=cd, out_scale=None):
        return be.call("gpk_sparse_propagate_multi", B, hs, 0, nx, coord, None, None, None, out_scale, hp(x1), 1,
                       hp(np.ascontiguousarray(U1[0])), 1, hp(lin), None, 1, None, R, H, hp(traj), hp(Sigma), None, None, None)

    entry()
    for what, msg, over in (("R = 33", r"R must be in \[1, 32\]", dict(R=33)), ("H = 257", r"H must be in \[1, 256\]", dict(H=257)),
                            ("H = 0", "H must be in", dict(H=0)), ("nx > D", "nx must be in", dict(nx=11)),
                            ("nx < B", "nx must be in", dict(nx=1)), ("B = 9", "1..8 models", dict(B=9)),
                            ("mismatched m", "m and D", dict(hs=handles(bg.models[0], other))),
                            ("a model that is not finalised", "finalised", dict(hs=handles(bg.models[0], raw))),
                            ("half an output scaler", "go together", dict(out_scale=hp(np.ones(2))))):
        with pytest.raises(_lib.GPKError, match=msg) as ei:
            entry(**over)
            pytest.fail(what)
        assert ei.value.code == _lib.GPK_BAD_ARG, what
    with pytest.raises(ValueError, match="m and D"):
        BatchedSparseGP([bg.models[0], other])
    # the single entry: no finalised object behind the handle
    with pytest.raises(_lib.GPKError, match="finalised") as ei:
        raw._backend().call("gpk_sparse_propagate", 0, hp(x1[:, :1].copy()), 1, hp(np.zeros((1, 5, 9))), 1, hp(lin[:1].copy()), None,
                            1, None, 1, 5, hp(np.empty((6, 1, 1))), hp(np.empty((6, 1, 1, 1))), None, None, None)
    assert ei.value.code == _lib.GPK_BAD_ARG
    # option small_path = 0: the predicate says so, route="chain" raises with the reason, the library refuses as well
    be.set_options(small_path=0)
    try:
        assert not bg.propagate_ok()
        with pytest.raises(ValueError, match="small_path"):
            bg.propagate(x1, U1, lin, route="chain", **kw)
        with pytest.raises(_lib.GPKError, match="small_path"):
            entry()
        same_bits("small_path = 0: auto is the host loop", bg.propagate(x1, U1, lin, **kw), bg.propagate(x1, U1, lin, route="host", **kw))
    finally:
        be.set_options(small_path=1)
    gp = served("single3")
    sbe = gp._backend()
    c3 = problem("single3")[0]
    one = gp.propagate(c3["x0"][0], c3["U"], c3["lin"], route="chain")
    sbe.set_options(small_path=0)
    try:
        assert not gp.propagate_ok()
        with pytest.raises(ValueError, match="small_path"):
            gp.propagate(c3["x0"][0], c3["U"], c3["lin"], route="chain")
    finally:
        sbe.set_options(small_path=1)
    x33, U33 = rollouts(c3["x0"][0], c3["U"], 33)
    with pytest.raises(ValueError, match="R must be in"):
        gp.propagate(x33, U33, c3["lin"], route="chain")
    with pytest.raises(ValueError, match="route must be"):
        gp.propagate(c3["x0"][0], c3["U"], c3["lin"], route="device")
    # the refusals left the handles serving: the same bits as before
    same_bits("single3 after the refusals", gp.propagate(c3["x0"][0], c3["U"], c3["lin"], route="chain"), one)
    same_bits("batch2 after the refusals", bg.propagate(x1, U1, lin, return_stages=True, route="chain", **kw), first)


# ---- 7. the control-loop wrappers take the chain ------------------------------------------------------------------------------------
def _advance_launches(be):
    """how many advance launches (GPK_TIMED_PROPAGATE brackets) the handle has recorded since its timing was switched on"""
    from unmanned_aerial_vehicles_amd import _lib
    ms, n = np.zeros(64), C.c_int(0)
    be.call("gpk_kernel_times", _lib.GPK_TIMED_PROPAGATE, _lib.host_ptr(ms), 64, C.byref(n))
    return n.value


def test_pretrained_gp_takes_the_chain_on_a_file_of_sparse_models(model_dict):
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    from test_gpu_sparse_batch import pretrained
    d, rows = model_dict
    pt = pretrained(d)
    bg = pt._fused()[0]
    assert isinstance(bg, BatchedSparseGP) and bg.propagate_ok()
    state, Ug, dt = rows[0, :6], np.ascontiguousarray(rows[:8, 6:].T), 0.02
    S0, Q = spd(6)
    be = bg._ensure()[0][0]
    be.call("gpk_timing", 1)
    try:
        assert _advance_launches(be) == 0
        X, Sig = pt.propagate_horizon(state, Ug, dt, Sigma0=S0, process_noise=Q)
        assert _advance_launches(be) == 8, "one advance launch per stage: the wrapper took the chain"
        be.call("gpk_timing", 1)      # (the ring starts again)
        be.set_options(small_path=0)
        try:
            wX, wS = pt.propagate_horizon(state, Ug, dt, Sigma0=S0, process_noise=Q)
        finally:
            be.set_options(small_path=1)
        assert _advance_launches(be) == 0, "small_path = 0: the wrapper took the host loop"
    finally:
        be.call("gpk_timing", 0)
    assert X.shape == (6, 9) and Sig.shape == (9, 6, 6)
    check("sparse file, the chain against the host loop: X", X, wX)
    check("sparse file, the chain against the host loop: Sigma", Sig, wS)


def test_simple_quadrotor_gp_takes_the_chain_with_a_sparse_model():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SimpleQuadrotorGP, SparseGP, WhiteKernel
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    rng = np.random.default_rng(77)
    n, m, H = 300, 60, 5
    X = rng.standard_normal((n, 10))
    Y = 0.2 * np.sin(X @ rng.standard_normal((10, 6)) / 2.0) + 0.02 * rng.standard_normal((n, 6))
    sp = SparseGP(ConstantKernel(0.9) * RBF(2.5 + 0.1 * np.arange(10)) + WhiteKernel(0.02), X[:m] + 0.05 * rng.standard_normal((m, 10)),
                  alpha=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0)).fit(X, Y)
    assert sp.propagate_ok()
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = sp, True
    state, Ug, dt = 0.3 * rng.standard_normal(6), 0.3 * rng.standard_normal((4, H)), 0.1
    _, lin = nominal_rollouts(sq._nominal_dynamics, state, Ug, dt, 1)
    S0, Q = spd(6)
    be = sp._backend()
    sp._ensure()
    be.call("gpk_timing", 1)
    try:
        Xh, Sig = sq.propagate_horizon(state, Ug, dt, Sigma0=S0, process_noise=Q)
        assert _advance_launches(be) == H, "one advance launch per stage: the wrapper took the chain"
    finally:
        be.call("gpk_timing", 0)
    assert Xh.shape == (6, H + 1) and Sig.shape == (H + 1, 6, 6) and sq.prediction_count == H
    wt, wS = sp.propagate(state, np.ascontiguousarray(Ug.T), lin, Sigma0=S0, process_noise=Q, route="host")
    check("propagate_horizon with a SparseGP against route = host: X", Xh, wt[:, 0].T)
    check("propagate_horizon with a SparseGP against route = host: Sigma", Sig, wS[:, 0])
    assert Sig[1:].any() and not np.array_equal(Xh[:, 1], state)
