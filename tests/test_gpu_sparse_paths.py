"""Posterior function draws of the sparse models ("the sparse models") on the GPU: `SparsePosteriorPaths` and
`BatchedSparsePosteriorPaths` - `paths(X)`, `step`, `rollout` - `SparseGP.sample_paths`, `BatchedSparseGP.sample_paths`,
`SimpleQuadrotorGP.sample_rollouts` with a `SparseGP` and `PreTrainedGP.sample_rollouts` on sparse models.  Buffers start out as
NaN (conftest: GPK_DEBUG_FILL), so a sum that ran into the padding of the set-up or between the models' column blocks would show.

Expected values: tests/golden/sparse_paths_ref.npz, the dense NumPy form of pathwise conditioning on the inducing variables with
explicit inverses (tests/golden/make_golden_sparse_paths.py, which also evaluates every case by solves against the factors: the
two agree to 1e-10 at cond(Kuu + jitter_uu I) <= 1e5 - measured 5e-16 .. 8e-13 at cond 5 .. 3.3e4).  Bar: 1e-8 of each array's
largest component, the bar of the sparse serving and the K10 tests.  Bit identity of the batch with the single-model path sets
is asserted with np.array_equal.

Cases, single (m, D, F, S, P, n): a (40, 4, 48, 5, 1, 150); b (50, 4, 64, 70, 3, 130): C = 210 crosses a 128-column tile, S
crosses 64; g (150, 4, 130, 3, 2, 300): m and F each cross one 128-tile.  Batch (m, D, F, S, B, n): c (64, 10, 96, 7, 6, 200): own
Z per model, input and target scalers, nx = 6, H = 25; d (33, 10, 32, 9, 4, 0): coord = (0, 2, 3, 5); e (16, 3, 16, 1, 1, 0);
f (20, 2, 16, 65, 8, 0): the largest B (no rollout: B > D).  Error growth of `rollout` in the NumPy form:
tests/test_sparse_paths_host.py."""
import importlib.util
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN, relerr

pytestmark = pytest.mark.gpu

FP64_BAR = 1e-8
SINGLE, BATCH = ("a", "b", "g"), ("c", "d", "e", "f")
ROLLOUT_BATCH = ("c", "d", "e")


def golden_module():
    spec = importlib.util.spec_from_file_location("make_golden_sparse_paths", os.path.join(GOLDEN, "make_golden_sparse_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = golden_module()


def check(tag, got, want, bar=FP64_BAR):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), tag
    e = relerr(got, want)
    print(f"{tag}: {e:.2e} (bar {bar:.1e})")
    assert e < bar, (tag, e)


def load_case(name):
    d = np.load(os.path.join(GOLDEN, "sparse_paths_ref.npz"))
    c = {k[len(name) + 1:]: d[k].astype(np.float64) for k in d.files if k.startswith(name + "_")}
    if "coord" in c:
        c["coord"] = c["coord"].astype(int)
    return c


def sparse_model(Z, X, Y, ls, hyper, y_mean, y_std):
    """a `SparseGP` at fixed hyper-parameters and normalisation, the rows (if any) taken in one `partial_fit`"""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    sf2, noise, alpha, jit = hyper
    sp = SparseGP(ConstantKernel(sf2) * RBF(ls) + WhiteKernel(noise), Z, alpha=alpha, jitter_uu=jit, y_mean=y_mean, y_std=y_std)
    if len(X):
        sp.partial_fit(X, Y[:, 0] if Y.shape[1] == 1 else Y)
    return sp


def shaped(a, P):
    """(M, S, P) of the form -> the package's shapes: (M, S) / (M, P, S) for `paths(X)`"""
    return a[:, :, 0] if P == 1 else a.transpose(0, 2, 1)


def squeezed(a, P):
    return a[..., 0] if P == 1 else a


_cases = {}


def case(name):
    """(inputs from the fixture, the model or batch, its path set, the NumPy form): built once, shared, left unchanged."""
    if name not in _cases:
        from unmanned_aerial_vehicles_amd import BatchedSparseGP, BatchedSparsePosteriorPaths, SparsePosteriorPaths
        c = load_case(name)
        if name in SINGLE:
            sp = sparse_model(c["Z"], c["X"], c["Y"], c["ls"], c["hyper"], c["ynorm"][0], c["ynorm"][1])
            paths = SparsePosteriorPaths.from_randomness(sp, c["omega"], c["phase"], c["weights"], c["xi"])
            form = G.SparseForm(c["Z"], c["X"], c["Y"], c["ls"], *c["hyper"], c["ynorm"][0], c["ynorm"][1], c["omega"], c["phase"],
                                c["weights"], c["xi"])
            _cases[name] = (c, sp, paths, form)
        else:
            B = len(c["ls"])
            bg = BatchedSparseGP([sparse_model(c["Z"][b], c["X"], c["Y"][:, b:b + 1], c["ls"][b], c["hyper"][b], c["ynorm"][0, b:b + 1],
                                               c["ynorm"][1, b:b + 1]) for b in range(B)])
            paths = BatchedSparsePosteriorPaths.from_randomness(bg, c["omega"], c["phase"], c["weights"], c["xi"])
            paths.set_output_scaler(c["out"][0], c["out"][1])
            form = G.SparseBatchForm(c["Z"], c["X"], c["Y"], c["ls"], c["hyper"], c["ynorm"], c["omega"], c["phase"], c["weights"],
                                     c["xi"], c["out"])
            _cases[name] = (c, bg, paths, form)
    return _cases[name]


def roll(paths, c, **over):
    a = dict(x0=c["x0"], U=c["U"], lin=c["lin"], coord=c["coord"], in_scaler=(c["in"][0], c["in"][1]))
    a.update(over)
    return paths.rollout(a["x0"], a["U"], a["lin"], coord=a["coord"], in_scaler=a["in_scaler"])


# ---- 1. parity with the fixture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE)
def test_single_model_against_the_fixture(name):
    c, sp, paths, form = case(name)
    m, F, S, P = len(c["Z"]), len(c["omega"]), c["weights"].shape[1], c["weights"].shape[2]
    assert paths.coef.shape == (m + F, S * P) and np.isfinite(paths.coef.cpu().numpy()).all()
    assert np.array_equal(paths._X.cpu().numpy(), c["Z"]), "the path set's own copy of the inducing inputs"
    check(f"case {name}: NumPy form against the fixture", form.all(c["Xq"]), c["all"], 1e-11)
    check(f"case {name}: paths(X)", paths(c["Xq"]), shaped(c["all"], P))
    check(f"case {name}: step", paths.step(c["Xs"]), squeezed(c["step"], P))
    got = paths.rollout(c["x0"], c["U"], c["lin"])
    assert (got[0] == c["x0"]).all()
    check(f"case {name}: rollout", got, c["traj"])
    a, b = paths.step(c["Xs"]), paths.step(c["Xs"])
    assert a.tobytes() == b.tobytes(), "the same bits every call"


@pytest.mark.parametrize("name", BATCH)
def test_batch_against_the_fixture(name):
    c, bg, paths, form = case(name)
    B, S = c["weights"].shape[0], c["weights"].shape[2]
    m, F = c["Z"].shape[1], c["omega"].shape[1]
    assert paths.mstride % 8 == 0 and paths.mstride >= S and paths.coef.shape == (m + F, B * paths.mstride)
    assert np.array_equal(paths._X.cpu().numpy(), c["Z"]), "the path set's own copies of the inducing inputs"
    check(f"case {name}: NumPy form against the fixture", form.all(c["Xq"]), c["all"], 1e-11)
    check(f"case {name}: paths(X)", paths(c["Xq"]), c["all"])
    check(f"case {name}: step", paths.step(c["Xs"]), c["step"])
    a, b = paths.step(c["Xs"]), paths.step(c["Xs"])
    assert a.tobytes() == b.tobytes(), "the same bits every call"
    if name in ROLLOUT_BATCH:
        got = roll(paths, c)
        assert got.shape == c["traj"].shape and (got[0] == c["x0"]).all()
        check(f"case {name}: rollout", got, c["traj"])
        assert roll(paths, c).tobytes() == got.tobytes()
        # a coordinate without a model follows lin alone
        nx = c["x0"].shape[1]
        free = [i for i in range(nx) if i not in set(c["coord"].tolist())]
        assert (name != "d") or free == [1, 4]
        for h, u in enumerate(c["U"]):
            q = np.concatenate([got[h], np.broadcast_to(u, (S, len(u)))], axis=1)
            for i in free:
                assert np.max(np.abs(got[h + 1][:, i] - (got[h][:, i] + q @ c["lin"][i]))) <= 1e-12 * np.max(np.abs(got)), (name, h, i)


# ---- 2. anchors against code that exists ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE + BATCH)
def test_zero_randomness_is_the_sparse_posterior_mean(name):
    from unmanned_aerial_vehicles_amd import BatchedSparsePosteriorPaths, SparsePosteriorPaths
    c, model, _, _ = case(name)
    cls = SparsePosteriorPaths if name in SINGLE else BatchedSparsePosteriorPaths
    zero = cls.from_randomness(model, c["omega"], c["phase"], np.zeros_like(c["weights"]), np.zeros_like(c["xi"]))
    mean = model.predict(c["Xq"])
    S = zero.S
    if name in SINGLE and zero.P == 1:
        want = np.repeat(mean[:, None], S, axis=1)
    else:
        want = np.repeat(mean[:, :, None], S, axis=2)
    check(f"case {name}: all {S} paths with xi = 0, w = 0 against predict", zero(c["Xq"]), want)
    if S <= 9:
        check(f"case {name}: step with xi = 0, w = 0 against predict", zero.step(c["Xq"][:S]), mean[:S])


def test_inducing_inputs_at_the_rows_give_the_exact_mean():
    """Z = X under the exact model's kernel: the sparse model is the exact GP, and its paths with xi = 0, w = 0 are its mean."""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, SparseGP, SparsePosteriorPaths, WhiteKernel
    c = load_case("a")
    X, Xq = c["Z"], c["Xq"]
    y = np.sin(X @ np.array([0.5, -0.3, 0.2, 0.4])) + 0.1 * np.cos(3.0 * X[:, 0]) + 1.5
    exact = GaussianProcessRegressor(ConstantKernel(0.9) * RBF(c["ls"]) + WhiteKernel(0.05), alpha=1e-4, normalize_y=True,
                                     optimizer=None).fit(X, y)
    sp = SparseGP.from_exact(exact, inducing=None, jitter_uu=1e-12).partial_fit(X, y)
    zero = SparsePosteriorPaths.from_randomness(sp, c["omega"], c["phase"], np.zeros((48, 4, 1)), np.zeros((40, 4, 1)))
    want = exact.predict(Xq)
    check("Z = X: paths with xi = 0, w = 0 against the exact GP's mean", zero(Xq), np.repeat(want[:, None], 4, axis=1))
    check("Z = X: step against the exact GP's mean", zero.step(Xq[:4]), want[:4])


# ---- 3. the bits of the single-model path sets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c", "e", "f"))
def test_every_model_has_the_bits_of_its_own_path_set(name):
    from unmanned_aerial_vehicles_amd import BatchedSparsePosteriorPaths, SparsePosteriorPaths
    c, bg, cached, _ = case(name)
    B, S = c["weights"].shape[0], c["weights"].shape[2]
    batch = BatchedSparsePosteriorPaths.from_randomness(bg, c["omega"], c["phase"], c["weights"], c["xi"])       # no output scaler
    coef = batch.coef.cpu().numpy()
    assert np.array_equal(coef, cached.coef.cpu().numpy(), equal_nan=True), "two set-ups differ"
    step = batch.step(c["Xs"])
    assert step.shape == (S, B) and np.isfinite(step).all()
    for b in range(B):
        single = SparsePosteriorPaths.from_randomness(bg.models[b], c["omega"][b], c["phase"][b], c["weights"][b], c["xi"][b])
        block = coef[:, b * batch.mstride:b * batch.mstride + S]
        assert np.isfinite(block).all()
        assert np.array_equal(block, single.coef.cpu().numpy()), f"case {name}: the column block of model {b}"
        assert np.array_equal(step[:, b], single.step(c["Xs"])), f"case {name}: column {b} of step"
    # the padding between the blocks is nobody's: still the NaN it was allocated with after the B set-ups
    assert batch.mstride > S
    assert np.isnan(coef.reshape(len(coef), B, batch.mstride)[:, :, S:]).all()


# ---- 4. sample_paths ---------------------------------------------------------------------------------------------------------------
def test_sample_paths_is_seeded():
    from unmanned_aerial_vehicles_amd import draw_sparse_batch_path_randomness, draw_sparse_path_randomness
    c, sp, _, _ = case("b")                    # (m, D, P) = (50, 4, 3)
    p1, p2 = sp.sample_paths(6, n_features=40, random_state=3), sp.sample_paths(6, n_features=40, random_state=3)
    assert p1.coef.shape == (50 + 40, 18)
    c1 = p1.coef.cpu().numpy()
    assert np.isfinite(c1).all() and np.array_equal(c1, p2.coef.cpu().numpy())
    assert not np.array_equal(c1, sp.sample_paths(6, n_features=40, random_state=4).coef.cpu().numpy())
    r = draw_sparse_path_randomness(np.random.RandomState(3), 50, 4, 40, 6, 3, c["ls"])
    for k in ("omega", "phase", "weights", "xi"):
        assert np.array_equal(p1.randomness[k], r[k]), k
    form = G.SparseForm(c["Z"], c["X"], c["Y"], c["ls"], *c["hyper"], c["ynorm"][0], c["ynorm"][1], r["omega"], r["phase"],
                        r["weights"], r["xi"])
    check("SparseGP.sample_paths(6, 40, 3) against the NumPy form", p1(c["Xq"]), shaped(form.all(c["Xq"]), 3))
    c, bg, _, _ = case("d")                    # (m, D, B) = (33, 10, 4)
    p1, p2 = bg.sample_paths(6, n_features=40, random_state=3), bg.sample_paths(6, n_features=40, random_state=3)
    assert p1.coef.shape == (33 + 40, 4 * 8) and p1.mstride == 8
    c1 = p1.coef.cpu().numpy()
    assert np.isfinite(c1.reshape(73, 4, 8)[:, :, :6]).all() and np.array_equal(c1, p2.coef.cpu().numpy(), equal_nan=True)
    r = draw_sparse_batch_path_randomness(np.random.RandomState(3), 33, 10, 40, 6, c["ls"])
    for k in ("omega", "phase", "weights", "xi"):
        assert np.array_equal(p1.randomness[k], r[k]), k
    form = G.SparseBatchForm(c["Z"], c["X"], c["Y"], c["ls"], c["hyper"], c["ynorm"], r["omega"], r["phase"], r["weights"], r["xi"])
    check("BatchedSparseGP.sample_paths(6, 40, 3) against the NumPy form", p1(c["Xq"]), form.all(c["Xq"]))


# ---- 5. the two sample_rollouts --------------------------------------------------------------------------------------------------------
def double_integrator(dt):
    lin = np.zeros((6, 10))
    lin[0:3, 3:6] = dt * np.eye(3)
    lin[3:6, 6:9] = dt * np.eye(3)
    return lin


def test_simple_quadrotor_gp_sample_rollouts_with_a_sparse_model(capsys):
    from unmanned_aerial_vehicles_amd import SimpleQuadrotorGP, draw_sparse_path_randomness
    c = load_case("c")                          # rows (200, 10), targets (200, 6): one six-output model on model 0's kernel and Z
    dt, R, F, H = 0.02, 5, 32, 25
    hyper, ym, ys = c["hyper"][0], c["ynorm"][0], c["ynorm"][1]
    n0 = 120
    sp = sparse_model(c["Z"][0], c["X"][:n0], c["Y"][:n0], c["ls"][0], hyper, ym, ys)
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = sp, True
    state, U_guess = 0.3 * c["Xq"][0, :6], 0.3 * c["Xq"][:4, 6:].T @ np.ones((4, H)) / 4.0 + 0.1 * np.sin(np.arange(H))[None]
    lin = double_integrator(dt)

    def want(rows):
        r = draw_sparse_path_randomness(np.random.RandomState(7), 64, 10, F, R, 6, c["ls"][0])
        form = G.SparseForm(c["Z"][0], c["X"][:rows], c["Y"][:rows], c["ls"][0], *hyper, ym, ys, r["omega"], r["phase"],
                            r["weights"], r["xi"])
        return form.rollout(state, U_guess.T, lin).transpose(1, 2, 0)

    capsys.readouterr()
    got = sq.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7)
    assert "failed" not in capsys.readouterr().out
    assert got.shape == (R, 6, H + 1) and all((got[r, :, 0] == state).all() for r in range(R))
    check("SimpleQuadrotorGP.sample_rollouts with a SparseGP against the NumPy rollout", got, want(n0))
    assert not np.allclose(got[0], got[1], rtol=0, atol=1e-9), "the rollouts differ: each follows its own function"
    cached = sq._paths[1]
    again = sq.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7)
    assert sq._paths[1] is cached and again.tobytes() == got.tobytes()
    # the model takes rows: the cached set is a snapshot of the old model and is drawn again
    sp.partial_fit(c["X"][n0:], c["Y"][n0:])
    new = sq.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7)
    assert sq._paths[1] is not cached
    check("... after partial_fit against the NumPy rollout of the updated model", new, want(200))
    assert relerr(new, got) > 1e-6, "the update must be visible"
    # a failure never reaches the control loop
    capsys.readouterr()
    bad = sq.sample_rollouts(state, np.full((4, H), np.nan), dt, n_rollouts=R, n_features=F, random_state=7)
    assert bad.shape == (R, 6, H + 1) and "GP rollout sampling failed" in capsys.readouterr().out
    bad = sq.sample_rollouts(state, U_guess, dt, n_rollouts=5000, n_features=F, random_state=7)
    assert bad.shape == (5000, 6, H + 1) and "GP rollout sampling failed" in capsys.readouterr().out
    assert all((bad[r] == bad[0]).all() for r in (1, 4999)) and np.isfinite(bad).all()


def trainer_dict(c, models, keep):
    from unmanned_aerial_vehicles_amd.trainer import OUTPUT_NAMES, StandardScaler
    sx = StandardScaler()
    sx.mean_, sx.scale_ = c["in"][0].copy(), c["in"][1].copy()
    d = {"gp_models": {}, "scalers_X": {}, "scalers_y": {}, "training_stats": {}}
    for b in keep:
        sy = StandardScaler()
        sy.mean_, sy.scale_ = c["out"][0][b:b + 1].copy(), c["out"][1][b:b + 1].copy()
        d["gp_models"][OUTPUT_NAMES[b]], d["scalers_X"][OUTPUT_NAMES[b]], d["scalers_y"][OUTPUT_NAMES[b]] = models[b], sx, sy
    return d


def test_pretrained_gp_sample_rollouts_on_sparse_models(capsys):
    from unmanned_aerial_vehicles_amd import PreTrainedGP, draw_sparse_batch_path_randomness
    c = load_case("c")
    dt, R, F, H = 0.02, 5, 32, 25
    n0 = 120
    models = [sparse_model(c["Z"][b], c["X"][:n0], c["Y"][:n0, b:b + 1], c["ls"][b], c["hyper"][b], c["ynorm"][0, b:b + 1],
                           c["ynorm"][1, b:b + 1]) for b in range(6)]
    state, U_guess = c["x0"][0], c["U"].T                       # (6,), (4, 25)
    pg = PreTrainedGP("/nonexistent/model.pkl")
    capsys.readouterr()
    nominal = pg.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F)
    assert nominal.shape == (R, 6, H + 1) and all((nominal[r] == nominal[0]).all() for r in range(R))
    assert "GP rollout sampling failed: no models are loaded" in capsys.readouterr().out

    def want(keep, rows):
        r = draw_sparse_batch_path_randomness(np.random.RandomState(7), 64, 10, F, R, c["ls"][keep])
        form = G.SparseBatchForm(c["Z"][keep], c["X"][:rows], c["Y"][:rows][:, keep], c["ls"][keep], c["hyper"][keep],
                                 c["ynorm"][:, keep], r["omega"], r["phase"], r["weights"], r["xi"],
                                 (c["out"][0][keep], c["out"][1][keep]))
        return form.rollout(state, c["U"], c["lin"], keep, (c["in"][0], c["in"][1])).transpose(1, 2, 0)

    for keep in (list(range(6)), [0, 2, 3, 4, 5]):
        d = trainer_dict(c, models, keep)
        if len(keep) == 6:      # as read back from a model file: the statistics travel, the device state is rebuilt
            d = pickle.loads(pickle.dumps(d))
        assert pg.load_dict(d) and pg._axis_paths is None
        capsys.readouterr()
        got = pg.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7)
        assert "failed" not in capsys.readouterr().out
        assert got.shape == (R, 6, H + 1) and all((got[r, :, 0] == state).all() for r in range(R)), "stage 0 is the state"
        check(f"sample_rollouts with sparse models {keep} against the NumPy rollout", got, want(keep, n0))
        assert not np.allclose(got[0], got[1], rtol=0, atol=1e-9), "the rollouts differ: each follows its own functions"
        if len(keep) < 6:     # the coordinate without a model is the nominal one given the others
            assert np.max(np.abs(got[:, 1, 1:] - (got[:, 1, :-1] + dt * got[:, 4, :-1]))) < 1e-12
        cached = pg._axis_paths[1]
        again = pg.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7)
        assert pg._axis_paths[1] is cached and again.tobytes() == got.tobytes()
    # one model takes rows: the next call draws a new set, of the updated models
    models[3].partial_fit(c["X"][n0:], c["Y"][n0:, 3])
    new = pg.sample_rollouts(state, U_guess, dt, n_rollouts=R, n_features=F, random_state=7)
    assert pg._axis_paths[1] is not cached
    keep = [0, 2, 3, 4, 5]
    r = draw_sparse_batch_path_randomness(np.random.RandomState(7), 64, 10, F, R, c["ls"][keep])
    forms = G.SparseBatchForm(c["Z"][keep], c["X"][:n0], c["Y"][:n0][:, keep], c["ls"][keep], c["hyper"][keep], c["ynorm"][:, keep],
                              r["omega"], r["phase"], r["weights"], r["xi"], (c["out"][0][keep], c["out"][1][keep]))
    forms.forms[2] = G.SparseBatchForm(c["Z"][[3]], c["X"], c["Y"][:, [3]], c["ls"][[3]], c["hyper"][[3]], c["ynorm"][:, [3]],
                                       r["omega"][[2]], r["phase"][[2]], r["weights"][[2]], r["xi"][[2]]).forms[0]
    check("... after partial_fit on one model against the NumPy rollout of the updated models", new,
          forms.rollout(state, c["U"], c["lin"], keep, (c["in"][0], c["in"][1])).transpose(1, 2, 0))
    assert relerr(new, got) > 1e-9, "the update must be visible"
    # a failure never reaches the control loop: the nominal trajectory, and a printed line
    capsys.readouterr()
    bad = pg.sample_rollouts(state, np.full((4, H), np.nan), dt, n_rollouts=R, n_features=F, random_state=7)
    assert bad.shape == (R, 6, H + 1) and "GP rollout sampling failed" in capsys.readouterr().out
    bad = pg.sample_rollouts(state, U_guess, dt, n_rollouts=5000, n_features=F, random_state=7)
    assert bad.shape == (5000, 6, H + 1) and "GP rollout sampling failed" in capsys.readouterr().out
    assert (bad[0] == nominal[0]).all()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_limits_and_shapes_raise_value_errors():
    from unmanned_aerial_vehicles_amd import BatchedSparsePosteriorPaths, SparsePosteriorPaths
    c, sp, paths, _ = case("a")                       # (m, D, F, S, P) = (40, 4, 48, 5, 1)
    om, ph, w, x = c["omega"], c["phase"], c["weights"], c["xi"]
    for n_paths, n_features in ((0, 16), (4097, 16), (2, 0), (2, 16385)):
        with pytest.raises(ValueError):
            sp.sample_paths(n_paths, n_features=n_features)
    for bad in ((om[:, :2], ph, w, x), (om, ph[:-1], w, x), (om, ph, w[:-1], x), (om, ph, w, x[:-1]), (om, ph, w, x[:, :-1]),
                (om, ph, np.where(w == w[0, 0, 0], np.nan, w), x), (om, ph, w, np.where(x == x[0, 0, 0], np.inf, x))):
        with pytest.raises(ValueError):
            SparsePosteriorPaths.from_randomness(sp, *bad)
    for bad in (c["Xs"][:, :2], np.concatenate([c["Xs"], c["Xs"]]), np.full_like(c["Xs"], np.nan)):
        with pytest.raises(ValueError):
            paths.step(bad)
    # a refused rollout leaves the path set usable
    for what, over in (("x0", dict(x0=np.zeros((2, 1)))), ("U must be", dict(U=c["U"][:, :1])), ("lin", dict(lin=c["lin"][:, :2])),
                       ("horizon", dict(U=np.zeros((257, 3)))), ("NaN or infinity", dict(U=np.full_like(c["U"], np.nan)))):
        a = dict(x0=c["x0"], U=c["U"], lin=c["lin"])
        a.update(over)
        with pytest.raises(ValueError, match=what):
            paths.rollout(**a)
    check("step after the refusals", paths.step(c["Xs"]), c["step"][:, 0])
    check("rollout after the refusals", paths.rollout(c["x0"], c["U"], c["lin"]), c["traj"])
    c, bg, bpaths, _ = case("d")                      # (m, D, F, S, B) = (33, 10, 32, 9, 4)
    om, ph, w, x = c["omega"], c["phase"], c["weights"], c["xi"]
    for n_paths, n_features in ((0, 16), (4097, 16), (2, 0), (2, 16385)):
        with pytest.raises(ValueError):
            bg.sample_paths(n_paths, n_features=n_features)
    for bad in ((om[:, :, :2], ph, w, x), (om[:1], ph, w, x), (om, ph[:, :-1], w, x), (om, ph, w[:, :-1], x), (om, ph, w, x[:, :-1]),
                (om, ph, w, np.concatenate([x, x], axis=2)), (om, ph, w, np.where(x == x[0, 0, 0], np.inf, x))):
        with pytest.raises(ValueError):
            BatchedSparsePosteriorPaths.from_randomness(bg, *bad)
    for what, over in (("distinct", dict(coord=[1, 1, 2, 3])), ("coord must be in", dict(coord=[0, 1, 2, 6])),
                       ("NaN or infinity", dict(x0=np.full_like(c["x0"], np.nan))), ("horizon", dict(U=np.zeros((0, 4))))):
        with pytest.raises(ValueError, match=what):
            roll(bpaths, c, **over)
    check("batch step after the refusals", bpaths.step(c["Xs"]), c["step"])
    check("batch rollout after the refusals", roll(bpaths, c), c["traj"])


def test_the_c_entries_refuse_every_limit_before_any_launch():
    """GPK_BAD_ARG with its message from the three entries themselves, past the Python checks; the outputs - NaN before - are
    still NaN afterwards: nothing was launched or copied."""
    import ctypes as C
    from unmanned_aerial_vehicles_amd import RBF, SparseGP, WhiteKernel, _lib
    from unmanned_aerial_vehicles_amd._lib import GPKError, dev_ptr as _p, host_ptr as _hp
    # the set-up, on case a's model: (m, D, F, S, P) = (40, 4, 48, 5, 1)
    c, sp, sp_paths, _ = case("a")
    be = sp._backend()
    w_d, x_d = be.upload(c["weights"].reshape(48, 5)), be.upload(c["xi"].reshape(40, 5))
    coef, zdst = be.empty((88, 5), w_d.dtype), be.empty((40, 4), w_d.dtype)

    def prep(**over):
        a = dict(omega=_p(sp_paths._omega), phase=_p(sp_paths._phase), F=48, w=_p(w_d), xi=_p(x_d), S=5, coef=_p(coef), ldc=5, z=_p(zdst))
        a.update(over)
        return tuple(a.values())

    for what, over in (("S must be in", dict(S=0)), ("S must be in", dict(S=4097, ldc=4097)), ("F must be in", dict(F=0)),
                       ("F must be in", dict(F=16385)), ("ldc must be", dict(ldc=4)), ("null pointer", dict(omega=None)),
                       ("null pointer", dict(phase=None)), ("null pointer", dict(w=None)), ("null pointer", dict(xi=None)),
                       ("null pointer", dict(coef=None)), ("null pointer", dict(z=None))):
        with pytest.raises(GPKError, match=what) as ei:
            be.call("gpk_sparse_paths_prepare", *prep(**over))
        assert ei.value.code == _lib.GPK_BAD_ARG, what
    be.call("gpk_batch_begin", 2)
    try:
        with pytest.raises(GPKError, match="batched mode"):
            be.call("gpk_sparse_paths_prepare", *prep())
    finally:
        be.status("gpk_batch_end")
    # a model that is not assembled: the refusal of gpk_sparse_predict
    raw = SparseGP(RBF(1.0) + WhiteKernel(0.1), c["Z"], alpha=1e-4)
    raw._begin(1)
    rbe = raw._backend()
    with pytest.raises(GPKError, match="no finalised sparse model") as ei:
        rbe.call("gpk_sparse_paths_prepare", *prep())
    assert ei.value.code == _lib.GPK_BAD_ARG
    # gpk_padded(m) + gpk_padded(F) > 65535 cannot be reached through a model: m <= 16384 and F <= 16384
    be.sync()
    rbe.sync()
    assert np.isnan(coef.cpu().numpy()).all() and np.isnan(zdst.cpu().numpy()).all(), "a refused set-up wrote its output"
    # the batch entries, on case d: (m, D, F, S, B) = (33, 10, 32, 9, 4), nx = 6
    c, bg, p, _ = case("d")
    be = p.be
    q = be.upload(c["Xs"])
    out = be.empty((p.S, p.B), q.dtype)
    x0, U, lin = (np.ascontiguousarray(c[k]) for k in ("x0", "U", "lin"))
    in_shift, in_scale = np.ascontiguousarray(c["in"][0]), np.ascontiguousarray(c["in"][1])
    traj = np.full((len(U) + 1, p.S, 6), np.nan)
    ints = lambda v: (C.c_int * len(v))(*v)      # noqa: E731

    def model(**over):
        a = dict(Zs=_p(p._X), N=p.N, D=p.D, B=p.B, ls=_hp(p._ls), sf2=_hp(p._sf2), omega=_p(p._omega), phase=_p(p._phase), F=p.F,
                 coef=_p(p.coef), ldc=p.ldc, mstride=p.mstride, S=p.S, shift=_hp(p._shift), scale=_hp(p._scale))
        a.update(over)
        return tuple(a.values())

    def tail(**over):
        a = dict(nx=6, coord=ints([0, 2, 3, 5]), in_shift=_hp(in_shift), in_scale=_hp(in_scale), x0=_hp(x0), x0_rows=p.S, U=_hp(U),
                 H=len(U), lin=_hp(lin), traj=_hp(traj))
        a.update(over)
        return tuple(a.values())

    bad_ls = p._ls.copy()
    bad_ls[1, 2] = -1.0
    zero_scale = in_scale.copy()
    zero_scale[3] = 0.0
    shared = (("B must be in", dict(B=0)), ("B must be in", dict(B=9)), ("D must be in", dict(D=17)), ("D must be in", dict(D=0)),
              ("S must be in", dict(S=4097, mstride=4104, ldc=16416)), ("S must be in", dict(S=0)),
              ("F must be in", dict(F=16385)), ("F must be in", dict(F=0)), ("N must be", dict(N=0)),
              ("mstride must be", dict(mstride=p.S - 1)), ("ldc must be", dict(ldc=p.B * p.mstride - 1)),
              ("length-scales must be positive", dict(ls=_hp(bad_ls))), ("null pointer", dict(coef=None)),
              ("null pointer", dict(Zs=None)))
    rollout_only = (("H must be in", dict(H=0)), ("H must be in", dict(H=257)), ("nx must be in", dict(nx=3)),
                    ("nx must be in", dict(nx=11)), ("1 or S rows", dict(x0_rows=2)),
                    ("coord must be distinct", dict(coord=ints([2, 2, 3, 5]))), ("coord must be in", dict(coord=ints([0, 2, 3, 6]))),
                    ("in_scale must be non-zero", dict(in_scale=_hp(zero_scale))), ("go together", dict(in_scale=None)),
                    ("null controls", dict(U=None)), ("NaN or infinity", dict(x0=_hp(np.full_like(x0, np.nan)))),
                    ("NaN or infinity", dict(U=_hp(np.full_like(U, np.inf)))), ("NaN or infinity", dict(lin=_hp(np.full_like(lin, np.nan)))),
                    ("null pointer", dict(traj=None)))
    calls = [("gpk_paths_step_multi_z", what, model(**over) + (_p(q), _p(out))) for what, over in shared]
    calls += [("gpk_paths_rollout_multi_z", what, model(**over) + tail()) for what, over in shared]
    calls += [("gpk_paths_rollout_multi_z", what, model() + tail(**over)) for what, over in rollout_only]
    for entry, what, args in calls:
        with pytest.raises(GPKError, match=what) as ei:
            be.call(entry, *args)
        assert ei.value.code == _lib.GPK_BAD_ARG, (entry, what)
    be.call("gpk_batch_begin", 2)
    try:
        for entry, args in (("gpk_paths_step_multi_z", model() + (_p(q), _p(out))), ("gpk_paths_rollout_multi_z", model() + tail())):
            with pytest.raises(GPKError, match="batched mode"):
                be.call(entry, *args)
    finally:
        be.status("gpk_batch_end")
    be.sync()
    assert np.isnan(out.cpu().numpy()).all() and np.isnan(traj).all(), "a refused call wrote its output"
    check("step after the refusals", p.step(c["Xs"]), c["step"])
