"""Greedy conditional-variance selection of inducing inputs on the GPU ("choosing Z") against
tests/golden/sparse_select_ref.npz and the NumPy recursion of its writer (tests/golden/make_golden_sparse_select.py): the
device-pointer building block `gpk_greedy_select`, the host entry `gpk_sparse_select` and the Python surface
(`SparseGP.select_inducing`, `from_exact(selection="greedy")`, `train(select_inducing="greedy")`).  Every buffer starts out as NaN
(indices as -1): what the call does not write is seen.

Bars: the recursion's rounding error in d is about t eps sf2 <= 1e-12 sf2 (the writer's docstring); trace and dmax are compared
at 1e-10 (of n sf2, of sf2), two orders over it.  On the tie-free cases the smallest gap between the two largest d is 6.6e-8 sf2,
four orders over the error, so the indices must be the fixture's exactly.  Where ties are real (many rows keep d == sf2 exactly)
no fixed sequence exists: the GPU's own sequence is judged by `follow` - at every step the row taken must be within 1e-9 sf2 of
the largest d of the NumPy recursion along that same sequence."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_sparse_select_host import load_select_writer

pytestmark = pytest.mark.gpu

TRACE_BAR = 1e-10      # of n sf2
DMAX_BAR = 1e-10       # of sf2
GREEDY_BAR = 1e-9      # of sf2: the row taken against the largest d of the reference recursion
MODEL_BAR = 1e-8       # of n sf2: the trace against the model's statistics (the project's fp64 bar)
CASES = ("A", "B", "C")


@pytest.fixture(scope="module")
def sref():
    d = np.load(os.path.join(GOLDEN, "sparse_select_ref.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def w():
    return load_select_writer()


@pytest.fixture(scope="module")
def be():
    from unmanned_aerial_vehicles_amd.device import Backend
    b = Backend(0)
    yield b
    b.lib.gpk_destroy(b.h)


class Result:
    def __init__(self, idx, trace, dmax, selected):
        self.idx, self.trace, self.dmax, self.selected = idx, trace, dmax, int(selected)

    def head(self):
        s = self.selected
        return self.idx[:s], self.trace[:s], self.dmax[:s]

    def untouched_past_selected(self):
        s = self.selected
        return bool(np.all(self.idx[s:] == -1) and np.isnan(self.trace[s:]).all() and np.isnan(self.dmax[s:]).all())


def device_select(be, X, ls, sf2, m_max, min_var=1e-10, tol=0.0):
    """gpk_greedy_select on device pointers; work area and outputs start as NaN / -1."""
    import torch
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, D = X.shape
    ls = np.ascontiguousarray(np.atleast_1d(ls), dtype=np.float64)
    nbytes = be.lib.gpk_greedy_select_bytes(n, m_max)
    assert nbytes >= 8 * (m_max + 17) * n and nbytes % 8 == 0
    dX = be.upload(X)
    work = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=be.device)
    idx = torch.full((m_max,), -1, dtype=torch.int64, device=be.device)
    trace = torch.full((m_max,), float("nan"), dtype=torch.float64, device=be.device)
    dmax = torch.full((m_max,), float("nan"), dtype=torch.float64, device=be.device)
    sel = torch.full((1,), -7, dtype=torch.int64, device=be.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with be.lock:
        be.bind_stream()
        be.check(be.lib.gpk_greedy_select(be.h, p(dX), n, D, ls.ctypes.data_as(C.POINTER(C.c_double)), ls.size, float(sf2), m_max,
                                          float(min_var), float(tol), p(work), p(idx), p(trace), p(dmax), p(sel)))
        be.sync()
    return Result(idx.cpu().numpy(), trace.cpu().numpy(), dmax.cpu().numpy(), sel.cpu().numpy()[0])


def sparse_model(X, ls, sf2, Z=None, noise=0.01):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    ls = np.atleast_1d(ls)
    kernel = ConstantKernel(sf2) * RBF(ls if ls.size > 1 else float(ls[0])) + WhiteKernel(noise)
    return SparseGP(kernel, X[:1] if Z is None else Z, alpha=1e-10)


def host_select(X, ls, sf2, m_max, min_var=1e-10, tol=0.0, held=False):
    """gpk_sparse_select under a sparse object's kernel: host rows, or (held) the rows that `hold` keeps."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    gp = sparse_model(X, ls, sf2)
    if held:
        gp.hold(X, np.zeros(len(X)))
    else:
        gp._begin(1)
    idx = np.full(m_max, -1, dtype=np.int64)
    trace, dmax = np.full(m_max, np.nan), np.full(m_max, np.nan)
    sel = C.c_int64(-7)
    b = gp._backend()
    dp = C.POINTER(C.c_double)
    with b.lock:
        b.bind_stream()
        b.check(b.lib.gpk_sparse_select(b.h, None if held else X.ctypes.data_as(dp), len(X), m_max, float(min_var), float(tol),
                                        idx.ctypes.data_as(C.POINTER(C.c_int64)), trace.ctypes.data_as(dp), dmax.ctypes.data_as(dp),
                                        C.byref(sel)))
    return Result(idx, trace, dmax, sel.value)


def check_greedy(w, X, ls, sf2, r, tag):
    """The GPU's own sequence judged by the NumPy recursion along it."""
    n = len(X)
    idx, trace, dmax = r.head()
    assert r.untouched_past_selected()
    assert len(set(idx.tolist())) == len(idx) and idx.min() >= 0 and idx.max() < n, "indices distinct and in range"
    d_before, tr = w.follow(X, ls, sf2, idx)
    taken = d_before[np.arange(len(idx)), idx]
    short = float(np.max(d_before.max(axis=1) - taken)) / sf2
    et = float(np.max(np.abs(trace - tr))) / (n * sf2)
    ed = float(np.max(np.abs(dmax - taken))) / sf2
    rise = float(np.max(np.diff(dmax), initial=0.0)) / sf2
    ties = int(np.sum(d_before[1] == sf2)) if len(idx) > 1 else 0
    print(f"{tag}: {len(idx)} rows; row taken short of the largest d by {short:.2e} sf2; trace {et:.2e} n sf2; dmax {ed:.2e} sf2; "
          f"largest rise of dmax {rise:.2e} sf2; rows with d == sf2 exactly at the second step: {ties}")
    assert short <= GREEDY_BAR
    assert et < TRACE_BAR and ed < DMAX_BAR
    assert rise <= DMAX_BAR
    return d_before


# ---- 1. exact sequence on the tie-free cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["device", "host", "held"])
@pytest.mark.parametrize("case", CASES)
def test_exact_sequence(be, sref, case, route):
    X, ls, sf2 = sref[f"{case}_X"], sref[f"{case}_ls"], float(sref["sf2"])
    m = len(sref[f"{case}_idx"])
    r = device_select(be, X, ls, sf2, m) if route == "device" else host_select(X, ls, sf2, m, held=route == "held")
    assert r.selected == m
    assert np.array_equal(r.idx, sref[f"{case}_idx"])
    et = float(np.max(np.abs(r.trace - sref[f"{case}_trace"]))) / (len(X) * sf2)
    ed = float(np.max(np.abs(r.dmax - sref[f"{case}_dmax"]))) / sf2
    print(f"case {case} ({route}): trace {et:.2e} n sf2, dmax {ed:.2e} sf2")
    assert et < TRACE_BAR and ed < DMAX_BAR


# ---- 2. greedy optimality where ties are real -----------------------------------------------------------------------------
def tie_case(name, csv_data):
    rng = np.random.default_rng(861)
    if name == "n1300":
        return rng.standard_normal((1300, 9)), np.exp(rng.uniform(-0.3, 0.5, 9)), 130
    if name == "csv":
        return np.ascontiguousarray(csv_data["X10"][:, :9]), np.array([0.11]), 256
    if name == "n37":
        return rng.standard_normal((37, 1)), np.array([0.7]), 37
    if name == "D16":
        return rng.standard_normal((500, 16)), np.exp(rng.uniform(-0.3, 0.5, 16)), 40
    if name == "n70001":      # 137 workgroup partials (more than one wave reduces), n a multiple of nothing
        return rng.standard_normal((70001, 3)), np.exp(rng.uniform(-0.3, 0.5, 3)), 40
    if name == "n1048583":    # past 2048 x 512 rows: two passes per workgroup, 1025 partials
        return rng.standard_normal((1048583, 2)), np.exp(rng.uniform(-0.3, 0.5, 2)), 6
    raise KeyError(name)


@pytest.mark.parametrize("name", ["n1300", "csv", "n37", "D16", "n70001", "n1048583"])
def test_greedy_where_ties_are_real(be, w, csv_data, name):
    X, ls, m = tie_case(name, csv_data)
    sf2 = 1.0 if name == "csv" else 1.3
    r = device_select(be, X, ls, sf2, m)
    check_greedy(w, X, ls, sf2, r, name)
    if name != "n37":
        assert r.selected == m
        return
    # m_max = n: every row, unless the rows left fall under the variance floor - then they all do
    assert 1 <= r.selected <= 37
    if r.selected < 37:
        left = [i for i in range(37) if i not in set(r.idx[:r.selected].tolist())]
        d_after = w.follow(X, ls, sf2, list(r.idx[:r.selected]) + left[:1])[0][-1]
        print(f"n37: stopped after {r.selected} rows with the largest d left {d_after.max() / sf2:.2e} sf2")
        assert d_after.max() <= (1e-10 + GREEDY_BAR) * sf2


# ---- 3. duplicates ---------------------------------------------------------------------------------------------------------
def test_duplicated_rows_are_never_both_selected(be, sref, w):
    X0, ls, sf2 = sref["B_X"], sref["B_ls"], float(sref["sf2"])
    X = np.vstack([X0, X0[:50]])
    r = device_select(be, X, ls, sf2, 130)
    check_greedy(w, X, ls, sf2, r, "B with its first 50 rows appended again")
    chosen = set(r.idx[:r.selected].tolist())
    both = [i for i in range(50) if i in chosen and 1500 + i in chosen]
    assert not both, f"row and copy both selected: {both}"
    assert r.selected == 130


def test_identical_rows_select_one(be, sref):
    X = np.tile(sref["B_X"][7:8], (333, 1))
    for r in (device_select(be, X, sref["B_ls"], 1.7, 20), host_select(X, sref["B_ls"], 1.7, 20)):
        assert r.selected == 1 and r.idx[0] == 0 and r.dmax[0] == 1.7
        assert 0.0 <= r.trace[0] <= 1e-10 * 333 * 1.7
        assert r.untouched_past_selected()


# ---- 4. stops --------------------------------------------------------------------------------------------------------------
def test_stops(be, sref):
    X, ls, sf2 = sref["A_X"], sref["A_ls"], float(sref["sf2"])
    n = len(X)
    tol = float(np.sqrt(sref["A_trace"][19] * sref["A_trace"][20])) / (n * sf2)
    for r in (device_select(be, X, ls, sf2, 64, tol=tol), host_select(X, ls, sf2, 64, tol=tol)):
        assert r.selected == 21
        assert r.untouched_past_selected(), "outputs past `selected` are not written"
        assert np.array_equal(r.idx[:21], sref["A_idx"][:21])
        assert np.max(np.abs(r.trace[:21] - sref["A_trace"][:21])) < TRACE_BAR * n * sf2
        assert np.max(np.abs(r.dmax[:21] - sref["A_dmax"][:21])) < DMAX_BAR * sf2
    # min_var between dmax[10] and dmax[11]: step 11 finds its largest d under the floor
    mv = float(np.sqrt(sref["A_dmax"][10] * sref["A_dmax"][11])) / sf2
    r = device_select(be, X, ls, sf2, 64, min_var=mv)
    assert r.selected == 11 and r.untouched_past_selected()
    assert np.array_equal(r.idx[:11], sref["A_idx"][:11])
    assert np.max(np.abs(r.trace[:11] - sref["A_trace"][:11])) < TRACE_BAR * n * sf2
    # one row: row 0, and the trace it leaves
    for r in (device_select(be, X, ls, sf2, 1), host_select(X, ls, sf2, 1)):
        assert r.selected == 1 and r.idx[0] == 0 and r.dmax[0] == sf2
        assert abs(r.trace[0] - sref["A_trace"][0]) < TRACE_BAR * n * sf2
    # a floor above sf2: nothing is selected, nothing is written
    r = device_select(be, X, ls, sf2, 8, min_var=1.5)
    assert r.selected == 0 and r.untouched_past_selected()


# ---- 5. determinism --------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(be, csv_data):
    X, ls, m = tie_case("csv", csv_data)
    a, b = device_select(be, X, ls, 1.0, m), device_select(be, X, ls, 1.0, m)
    assert a.selected == b.selected == m
    assert np.array_equal(a.idx, b.idx) and a.trace.tobytes() == b.trace.tobytes() and a.dmax.tobytes() == b.dmax.tobytes()


# ---- 6. consistency with the model -----------------------------------------------------------------------------------------
def test_trace_is_the_models_trace_term(be, sref):
    """n sf2 - tr(Kuu^-1 G) from the statistics of the sparse model on Z = X[idx] is the selection's last trace."""
    X, ls, sf2 = sref["C_X"], sref["C_ls"], float(sref["sf2"])
    n = len(X)
    r = device_select(be, X, ls, sf2, 200)
    Z = X[r.idx]
    gp = sparse_model(X, ls, sf2, Z=Z).fit(X, np.zeros(n))
    G = gp.statistics()["G"]
    e = (Z / ls)[:, None, :] - (Z / ls)[None, :, :]
    Kuu = sf2 * np.exp(-0.5 * np.sum(e * e, axis=2))
    got = n * sf2 - float(np.trace(np.linalg.solve(Kuu, G)))
    err = abs(got - r.trace[-1]) / (n * sf2)
    print(f"n sf2 - tr(Kuu^-1 G) = {got:.10e}, trace[-1] = {r.trace[-1]:.10e}: {err:.2e} n sf2")
    assert err < MODEL_BAR


# ---- 7. the Python surface -------------------------------------------------------------------------------------------------
def test_from_exact(sref):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, GaussianProcessRegressor, SparseGP, WhiteKernel
    X, ls, sf2 = sref["A_X"], sref["A_ls"], float(sref["sf2"])
    y = np.sin(X[:, 0]) + 0.1 * X[:, 1]
    kernel = ConstantKernel(sf2) * RBF(ls) + WhiteKernel(0.05)
    ex = GaussianProcessRegressor(kernel=kernel, alpha=1e-8, optimizer=None, device=0).fit(X, y)
    sp = SparseGP.from_exact(ex, inducing=64, selection="greedy")
    idx, trace = sparse_model(X, ls, sf2).select_inducing(X, 64)
    assert np.array_equal(idx, sref["A_idx"]) and np.array_equal(sp.inducing_, X[idx])
    assert trace.shape == (64,) and np.max(np.abs(trace - sref["A_trace"])) < TRACE_BAR * len(X) * sf2
    # the default: the seeded permutation, as before
    for rs in (0, 5):
        sp = SparseGP.from_exact(ex, inducing=64, random_state=rs)
        assert np.array_equal(sp.inducing_, X[np.sort(np.random.default_rng(rs).permutation(len(X))[:64])])
    # the sparse model on the greedy rows serves
    sp = SparseGP.from_exact(ex, inducing=64, selection="greedy").fit(X, y)
    assert np.sqrt(np.mean((sp.predict(X[:40]) - ex.predict(X[:40])) ** 2)) < 0.05 * y.std()
    # fewer usable rows than asked for
    dup = GaussianProcessRegressor(kernel=kernel, alpha=1e-2, optimizer=None, device=0).fit(np.tile(X[:3], (10, 1)), np.zeros(30))
    with pytest.raises(ValueError, match="usable rows"):
        SparseGP.from_exact(dup, inducing=5, selection="greedy")


def test_select_inducing_on_held_rows(sref):
    X, ls, sf2 = sref["A_X"], sref["A_ls"], float(sref["sf2"])
    gp = sparse_model(X, ls, sf2, Z=X[:64])
    gp.hold(X, np.zeros(len(X)))
    before = gp.statistics()
    idx, trace = gp.select_inducing()            # m: the object's, rows: the held ones
    assert np.array_equal(idx, sref["A_idx"]) and len(trace) == 64
    idx2, trace2 = gp.select_inducing(m=30, tol=float(np.sqrt(sref["A_trace"][19] * sref["A_trace"][20])) / (len(X) * sf2))
    assert np.array_equal(idx2, sref["A_idx"][:21]) and np.array_equal(trace2, trace[:21])
    after = gp.statistics()
    assert np.array_equal(gp.inducing_, X[:64]) and all(np.array_equal(before[k], after[k]) for k in ("G", "g", "yy"))
    with pytest.raises(ValueError):
        gp.select_inducing(m=len(X) + 1)


@pytest.mark.parametrize("train_z", [False, True], ids=["kernel", "kernel and Z"])
def test_train_reselects(train_z):
    from test_gpu_sparse_train import training_model
    d = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    ref = {k: d[k] for k in d.files}
    X, y = ref["T_X"], ref["T_Y"][:, 0]
    gp = training_model(ref)
    before = gp.hold(X, y).log_bound(gp.kernel_.theta)
    assert gp.train(X, y, select_inducing="greedy", selection_rounds=2, train_inducing=train_z) is gp
    print(f"bound {before:.6f} -> {gp.bound_value_:.6f}; kernel {gp.kernel_}")
    Z = gp.inducing_
    assert Z.shape == (64, 2) and len({tuple(z) for z in Z}) == 64, "64 distinct inducing inputs"
    if not train_z:
        rows = {tuple(x) for x in X}
        assert all(tuple(z) in rows for z in Z), "every inducing input is a row of X"
    else:
        assert not all(tuple(z) in {tuple(x) for x in X} for z in Z), "the last round moved Z"
    assert gp.bound_value_ == gp.log_bound() and np.isfinite(gp.bound_value_)
    assert gp.bound_value_ > before
    assert gp.n_rows_ == 600
