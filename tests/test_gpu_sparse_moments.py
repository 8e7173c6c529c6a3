"""Exact moment matching on the sparse posteriors (DESIGN.md, K11 "moment matching on the sparse models") on the GPU:
`SparseGP.predict_moments` / `propagate_moments` (`gpk_sparse_moments`, `gpk_sparse_propagate_mm`), their batch forms on
`BatchedSparseGP` (`gpk_sparse_moments_multi`, `gpk_sparse_propagate_mm_multi`), the query dimension of the pair launch and the
control-loop wrappers.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL), so a pair tile that read Q's padding, a row beyond m
or a slot that no group of queries wrote would show.

Expected values: `sparse_moments_numpy_form` of tests/test_sparse_moments_host.py (dense NumPy on (Z, alpha_u, Q), checked there
against Gauss-Hermite quadrature).  Bar: the project's fp64 bar, 1e-8 of each array's largest component; that file prints and
asserts what it rests on, at these queries (E[v] >= 3.6 % of the prior on every problem: the clip is inactive; float64 against
longdouble <= 5e-12).  Bit identity is asserted with np.array_equal.

Shapes: the problems of tests/test_sparse_propagate_host.py - single3 (m = 26, P = 3, D = 4: one tile), batch2 (B = 2, m = 60, nx =
6, both scalers: a = b and a != b pairs), batch8 (B = 8: 36 pairs, a permuted coord), one200 (m = 200: 10 lower tiles, rows 200 ..
255 of Q masked) - with H = 5 and R = 1, 5, 17, 32: with 256 CUs the pair launch takes min(R, 512 / (tiles x pairs)) groups of
queries - one group at R = 1, R groups of one query for single3, one200 and batch2, and for batch8 (36 workgroups) 14 groups over
17 or 32 queries, which do not divide."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_paths import check
from test_gpu_sparse_batch import model_dict  # noqa: F401  (the fixture: six sparse models behind one input scaler)
from test_gpu_sparse_propagate import _advance_launches, served
from test_propagate_host import rollouts, spd
from test_sparse_moments_host import gaussian_rows, model_defs, sparse_form, sparse_moments_numpy_form
from test_sparse_propagate_host import PROBLEMS, problem

pytestmark = pytest.mark.gpu

STAGES = ("mean", "cov", "xcov")


def scalers(name):
    kw = problem(name)[2]
    return {k: kw[k] for k in ("in_scaler", "out_scaler") if k in kw}


def backend_of(gp):
    """the serving backend: the model's own, or the first model's of a batch"""
    return gp._ensure()[0][0] if hasattr(gp, "models") else gp._backend()


def check_moments(tag, got, want):
    for what, g, w in zip(STAGES, got, want):
        check(f"{tag}: {what}", np.asarray(g), np.asarray(w))


def check_run(tag, got, want):
    for what, g, w in (("traj", got[0], want[0]), ("Sigma", got[1], want[1])) + tuple((k, got[2][k], want[2][k]) for k in STAGES):
        check(f"{tag}: {what}", g, w)


def same_bits(tag, a, b):
    assert np.array_equal(a[0], b[0]), f"{tag}: traj"
    assert np.array_equal(a[1], b[1]), f"{tag}: Sigma"
    if len(a) > 2:
        for k in STAGES:
            assert np.array_equal(a[2][k], b[2][k]), f"{tag}: {k}"


def same_moments(tag, a, b):
    for k, x, y in zip(STAGES, a, b):
        assert np.array_equal(x, y), f"{tag}: {k}"


# ---- 1. parity with the NumPy form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (1, 5, 17, 32))
@pytest.mark.parametrize("name", PROBLEMS)
def test_predict_moments_parity(name, R):
    c = problem(name)[0]
    gp, mform = served(name), sparse_form(name)
    nx, D = c["lin"].shape
    NO = mform.NO
    Q, S = gaussian_rows(name, R)
    for noisy in (False, True):
        got = gp.predict_moments(Q, S, var_includes_noise=noisy, **scalers(name))
        assert got[0].shape == (R, NO) and got[1].shape == (R, NO, NO) and got[2].shape == (R, NO, D)
        check_moments(f"{name}, R = {R}, noise {noisy}", got, mform.batch(Q, S, noisy))
        assert np.array_equal(got[1], got[1].transpose(0, 2, 1)), "every V block equals its transpose bit for bit"
        assert not got[2][:, :, nx:].any(), "the controls are certain"
        assert np.array_equal(got[0], gp.predict_moments(Q, S, var_includes_noise=noisy, **scalers(name))[0]), "a second call"


@pytest.mark.parametrize("R", (1, 5, 17, 32))
@pytest.mark.parametrize("name", PROBLEMS)
def test_propagate_moments_parity(name, R):
    c, _, kw, _ = problem(name)
    gp, mform = served(name), sparse_form(name)
    lin = c["lin"]
    nx, D = lin.shape
    coord = model_defs(name)[3]
    S0, Q = spd(nx)
    S0 = 0.05 * S0
    x0, U = rollouts(c["x0"][0], c["U"], R)
    H = U.shape[1]
    for noisy, extra, want_args in ((False, {}, (None, None)), (True, dict(Sigma0=S0, process_noise=Q), (np.tile(S0, (R, 1, 1)), Q))):
        got = gp.propagate_moments(x0, U, lin, var_includes_noise=noisy, return_stages=True, **kw, **extra)
        assert got[0].shape == (H + 1, R, nx) and got[1].shape == (H + 1, R, nx, nx) and got[2]["xcov"].shape == (H, R, mform.NO, D)
        assert np.array_equal(got[0][0], x0)
        check_run(f"{name}, R = {R}, noise {noisy}", got, mform.run(coord, x0, U, lin, *want_args, noisy=noisy))
    assert len(gp.propagate_moments(c["x0"][0], c["U"], lin, **kw)) == 2      # the shorthand shapes, no stages


# ---- 2. bits: stage outputs, rollouts, repeats, symmetry --------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_stage_outputs_have_the_bits_of_predict_moments(name):
    c, _, kw, _ = problem(name)
    gp = served(name)
    nx = c["lin"].shape[0]
    S0, Q = spd(nx)
    for R in (1, 17):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        for noisy in (False, True):
            traj, Sigma, st = gp.propagate_moments(x0, U, c["lin"], Sigma0=0.05 * S0, process_noise=Q, var_includes_noise=noisy,
                                                   return_stages=True, **kw)
            for h in range(U.shape[1]):
                q = np.ascontiguousarray(np.concatenate([traj[h], U[:, h]], axis=1))
                same_moments(f"{name}, R = {R}, stage {h}", [st[k][h] for k in STAGES],
                             gp.predict_moments(q, np.ascontiguousarray(Sigma[h]), var_includes_noise=noisy, **scalers(name)))


@pytest.mark.parametrize("name", PROBLEMS)
def test_rollouts_repeats_and_symmetry(name):
    c, _, kw, _ = problem(name)
    gp = served(name)
    nx = c["lin"].shape[0]
    S0, Q = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"], 17)
    args = dict(Sigma0=0.05 * S0, process_noise=Q, return_stages=True, **kw)
    full = gp.propagate_moments(x0, U, c["lin"], **args)
    same_bits(f"{name}: two calls", gp.propagate_moments(x0, U, c["lin"], **args), full)
    for r in (0, 9, 16):
        one = gp.propagate_moments(x0[r:r + 1], U[r:r + 1], c["lin"], **args)
        same_bits(f"{name}: rollout {r} of 17 against that rollout alone",
                  (full[0][:, r:r + 1], full[1][:, r:r + 1], {k: full[2][k][:, r:r + 1] for k in STAGES}), one)
    Sigma, cov = full[1], full[2]["cov"]
    assert np.array_equal(Sigma, Sigma.transpose(0, 1, 3, 2)), "every Sigma[h, r] equals its transpose bit for bit"
    assert np.array_equal(cov, cov.transpose(0, 1, 3, 2)), "every stage covariance equals its transpose bit for bit"
    ev, tr = np.linalg.eigvalsh(Sigma)[..., 0], np.trace(Sigma, axis1=2, axis2=3)
    assert (ev >= -1e-12 * tr).all()
    # Gaussian queries: row r of 17 against that row alone
    Qr, Sr = gaussian_rows(name, 17)
    all17 = gp.predict_moments(Qr, Sr, **scalers(name))
    for r in (0, 9, 16):
        same_moments(f"{name}: query {r} of 17 alone", [a[r:r + 1] for a in all17],
                     gp.predict_moments(Qr[r:r + 1], Sr[r:r + 1], **scalers(name)))


# ---- 3. the query dimension of the pair launch changes no bit ---------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_query_split_changes_no_bit(name):
    c, _, kw, _ = problem(name)
    gp = served(name)
    be = backend_of(gp)
    nx = c["lin"].shape[0]
    S0, Q = spd(nx)
    for R in (5, 17, 32):
        x0, U = rollouts(c["x0"][0], c["U"][:2], R)
        Qr, Sr = gaussian_rows(name, R)
        split = (gp.predict_moments(Qr, Sr, **scalers(name)),
                 gp.propagate_moments(x0, U, c["lin"], Sigma0=0.05 * S0, process_noise=Q, return_stages=True, **kw))
        for groups in (1, 3):
            be.set_options(moments_query_groups=groups)
            try:
                same_moments(f"{name}, R = {R}: at most {groups} group(s) against the default", gp.predict_moments(Qr, Sr, **scalers(name)),
                             split[0])
                same_bits(f"{name}, R = {R}: at most {groups} group(s) against the default",
                          gp.propagate_moments(x0, U, c["lin"], Sigma0=0.05 * S0, process_noise=Q, return_stages=True, **kw), split[1])
            finally:
                be.set_options(moments_query_groups=0)


def test_query_split_changes_no_bit_on_an_exact_model():
    from test_gpu_moments import problem as exact_problem
    c, gp, _ = exact_problem("b")
    S0, Q = spd(3)
    gp.predict_moments(np.zeros((1, 4)), None)      # (the device model exists)
    be = gp._dev.be
    for R in (5, 17, 32):
        x0, U = rollouts(c["x0"][0], c["U"], R)
        Qr = np.ascontiguousarray(np.concatenate([x0, U[:, 0]], axis=1))
        Sr = np.stack([S0 * (0.05 + 0.01 * r) for r in range(R)])
        kw = dict(Sigma0=0.05 * S0, process_noise=Q, return_stages=True, method="moment")
        split = gp.predict_moments(Qr, Sr), gp.propagate(x0, U, c["lin"], **kw)
        be.set_options(moments_query_groups=1)
        try:
            same_moments(f"exact model, R = {R}: one group against the default", gp.predict_moments(Qr, Sr), split[0])
            same_bits(f"exact model, R = {R}: one group against the default", gp.propagate(x0, U, c["lin"], **kw), split[1])
        finally:
            be.set_options(moments_query_groups=0)


# ---- 4. batching ---------------------------------------------------------------------------------------------------------------------
def test_one_model_batch_has_the_bits_of_the_single_model():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    c = problem("one200")[0]
    gp = served("one200")
    bg = BatchedSparseGP([gp])
    S0, Q = spd(1)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    Qr, Sr = gaussian_rows("one200", 17)
    for noisy in (False, True):
        same_moments(f"B = 1 against the model's own call, noise {noisy}", bg.predict_moments(Qr, Sr, var_includes_noise=noisy),
                     gp.predict_moments(Qr, Sr, var_includes_noise=noisy))
        args = dict(Sigma0=S0, process_noise=Q, var_includes_noise=noisy, return_stages=True)
        same_bits(f"B = 1 against the model's own chain, noise {noisy}", bg.propagate_moments(x0, U, c["lin"], **args),
                  gp.propagate_moments(x0, U, c["lin"], **args))


def test_column_b_of_eight_models_has_the_bits_of_model_b():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    c, _, kw, _ = problem("batch8")
    bg = served("batch8")
    Qr, Sr = gaussian_rows("batch8", 17)
    mean, cov, xcov = bg.predict_moments(Qr, Sr, var_includes_noise=True, **scalers("batch8"))
    for b in (0, 3, 7):
        out_b = (kw["out_scaler"][0][b:b + 1], kw["out_scaler"][1][b:b + 1])
        one = BatchedSparseGP([bg.models[b]]).predict_moments(Qr, Sr, in_scaler=kw["in_scaler"], out_scaler=out_b, var_includes_noise=True)
        assert np.array_equal(mean[:, b], one[0][:, 0]), (b, "mean")
        assert np.array_equal(cov[:, b, b], one[1][:, 0, 0]), (b, "cov")
        assert np.array_equal(xcov[:, b], one[2][:, 0]), (b, "xcov")


# ---- 5. the host loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("single3", "batch2"))
def test_host_route_agrees_with_the_chain(name):
    c, _, kw, _ = problem(name)
    gp = served(name)
    nx = c["lin"].shape[0]
    S0, Q = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    args = dict(Sigma0=0.05 * S0, process_noise=Q, return_stages=True, **kw)
    chain, host = gp.propagate_moments(x0, U, c["lin"], **args), gp.propagate_moments(x0, U, c["lin"], route="host", **args)
    for what, a, b in (("traj", chain[0], host[0]), ("Sigma", chain[1], host[1])) + tuple((k, chain[2][k], host[2][k]) for k in STAGES):
        check(f"{name}: chain against the host loop: {what}", a, b, 1e-10)


# ---- 6. Z = X: the sparse model is the exact one ---------------------------------------------------------------------------------
def test_inducing_inputs_at_the_rows_agree_with_the_exact_model():
    """Z = X and jitter_uu -> 0 make Q = (K + s2 I)^-1 and alpha_u = alpha: the exact model.  jitter_uu = 1e-10 here (Kuu of case
    b is positive definite on its own, smallest eigenvalue about 2e-7): small enough for the two MODELS to agree within 1.5e-9 -
    the gap of their NumPy forms, printed - so that 10 x the gap still reaches the cap of 1e-8, and twenty times above the
    1e-11 at which the float64 rounding of Q shows (tests/test_sparse_moments_host.py measures such forms against longdouble)."""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    from test_gpu_moments import problem as exact_problem
    c, gp, mform = exact_problem("b")
    sf2, noise, alpha = c["hyper"]
    jit = 1e-10
    sp = SparseGP(ConstantKernel(sf2) * RBF(c["ls"]) + WhiteKernel(noise), c["X"], alpha=alpha, jitter_uu=jit,
                  y_mean=c["Y"].mean(axis=0), y_std=c["Y"].std(axis=0)).fit(c["X"], c["Y"])
    sform = sparse_moments_numpy_form([dict(X=c["X"], Y=c["Y"], Z=c["X"], ls=c["ls"], sf2=sf2, noise=noise, alpha=alpha, jit=jit,
                                            ym=c["Y"].mean(axis=0), ys=c["Y"].std(axis=0))])
    S0, _ = spd(3)
    x0, U = rollouts(c["x0"][0], c["U"], 5)
    Qr = np.ascontiguousarray(np.concatenate([x0, U[:, 0]], axis=1))
    Sr = np.stack([S0 * (0.05 + 0.01 * r) for r in range(5)])
    for noisy in (False, True):
        gap = max(float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(sform.batch(Qr, Sr, noisy), mform.batch(Qr, Sr, noisy)))
        tol = min(10.0 * gap, 1e-8)
        print(f"Z = X, noise {noisy}: the two models' NumPy forms differ by {gap:.2e}; tolerance min(10 x that, 1e-8) = {tol:.2e}")
        got, want = sp.predict_moments(Qr, Sr, var_includes_noise=noisy), gp.predict_moments(Qr, Sr, var_includes_noise=noisy)
        for what, a, b in zip(STAGES, got, want):
            check(f"Z = X, noise {noisy}: SparseGP against GaussianProcessRegressor: {what}", a, b, tol)


# ---- 7. Q follows the model ---------------------------------------------------------------------------------------------------------
def test_q_is_refreshed_after_more_rows():
    from test_gpu_sparse_batch import ALPHA, build_model
    p = problem("one200")[0]["ps"][0]
    first = dict(p, X=p["X"][:200], y=p["y"][:200])
    gp = build_model(first)
    Qr, Sr = gaussian_rows("one200", 5)

    def form(q):
        return sparse_moments_numpy_form([dict(X=q["X"], Y=q["y"][:, None], Z=q["Z"], ls=q["ls"], sf2=q["sf2"], noise=q["noise"],
                                               alpha=ALPHA, jit=1e-8 * q["sf2"], ym=np.array([q["ym"]]), ys=np.array([q["ys"]]))])

    before = gp.predict_moments(Qr, Sr)
    check_moments("200 rows", before, form(first).batch(Qr, Sr, False))
    gp.partial_fit(p["X"][200:], p["y"][200:])
    after = gp.predict_moments(Qr, Sr)
    check_moments("300 rows: Q is that of all the rows", after, sparse_form("one200").batch(Qr, Sr, False))
    assert not np.array_equal(before[1], after[1])
    # (the statistics of 200 + 100 rows and of 300 rows at once differ in summation order)
    check_moments("against the model built on all rows at once", after, served("one200").predict_moments(Qr, Sr))


# ---- 8. the limits: refusals, and the same bits afterwards -----------------------------------------------------------------------
def test_limits_are_refused_and_leave_the_handle_serving():
    from unmanned_aerial_vehicles_amd import _lib
    from unmanned_aerial_vehicles_amd._lib import host_ptr as hp
    from test_gpu_sparse_batch import build_model, model_inputs
    c, _, kw, _ = problem("batch2")
    bg = served("batch2")
    lin = c["lin"]
    x1, U1 = rollouts(c["x0"][0], c["U"], 1)
    Q1, S1 = gaussian_rows("batch2", 1)
    first = bg.propagate_moments(x1, U1, lin, return_stages=True, **kw)
    firstq = bg.predict_moments(Q1, S1, **scalers("batch2"))
    raw = build_model(model_inputs(1, 60, 400, 10))        # rows, but never finalised
    bes, good = bg._ensure()
    be = bes[0]
    traj, Sigma = np.full((6, 1, 6), 7.0), np.full((6, 1, 6, 6), 7.0)
    mean, cov, xcov = np.full((1, 2), 7.0), np.full((1, 2, 2), 7.0), np.full((1, 2, 10), 7.0)
    cd = (C.c_int * 2)(*c["coord"])
    U0 = np.ascontiguousarray(U1[0])

    def handles(*gps):
        return (C.c_void_p * len(gps))(*[g._backend().h.value for g in gps])

    def chain(hs=good, B=2, nx=6, R=1, H=5, coord=cd, x0=x1, S0=None):
        return be.call("gpk_sparse_propagate_mm_multi", B, hs, 0, nx, coord, None, None, None, None, hp(x0), 1, hp(U0), 1, hp(lin),
                       hp(S0), 1, None, R, H, hp(traj), hp(Sigma), None, None, None)

    def query(hs=good, B=2, nx=6, M=1, Xq=Q1, Sq=S1):
        return be.call("gpk_sparse_moments_multi", B, hs, 0, nx, None, None, None, None, hp(Xq), hp(Sq), M, hp(mean), hp(cov), hp(xcov))

    nanq, nans, nanx = Q1.copy(), S1.copy(), x1.copy()
    nanq[0, 9], nans[0, 5, 5], nanx[0, 0] = np.nan, np.inf, np.nan
    for what, msg, call in (
            ("M = 33", r"M must be in \[1, 32\]", lambda: query(M=33)), ("M = 0", "M must be in", lambda: query(M=0)),
            ("R = 33", r"R must be in \[1, 32\]", lambda: chain(R=33)), ("H = 257", r"H must be in \[1, 256\]", lambda: chain(H=257)),
            ("nx = 17", "nx <= D <= 16", lambda: query(nx=17)), ("nx > D", "nx <= D <= 16", lambda: query(nx=11)),
            ("nx > D in the chain", "nx <= D <= 16", lambda: chain(nx=11)),
            ("nx below the number of outputs", "must not be below the number of outputs", lambda: chain(nx=1)),
            ("coord out of range", r"coord must be in \[0, nx\)", lambda: chain(coord=(C.c_int * 2)(4, 6))),
            ("coord repeated", "coord must be distinct", lambda: chain(coord=(C.c_int * 2)(1, 1))),
            ("NaN in a query", "NaN or infinity", lambda: query(Xq=nanq)), ("infinity in a covariance", "NaN or infinity", lambda: query(Sq=nans)),
            ("NaN in x0", "NaN or infinity", lambda: chain(x0=nanx)), ("B = 9", "1..8 models", lambda: query(B=9)),
            ("a model that is not finalised", "finalised", lambda: query(hs=handles(bg.models[0], raw))),
            ("a model that is not finalised, the chain", "finalised", lambda: chain(hs=handles(bg.models[0], raw)))):
        with pytest.raises(_lib.GPKError, match=msg) as ei:
            call()
            pytest.fail(what)
        assert ei.value.code == _lib.GPK_BAD_ARG, what
    # the single entries: no finalised object behind the handle
    for entry, args in (("gpk_sparse_moments", (0, 1, hp(Q1), None, 1, hp(mean), hp(cov), hp(xcov))),
                        ("gpk_sparse_propagate_mm", (0, hp(x1[:, :1].copy()), 1, hp(np.zeros((1, 5, 9))), 1, hp(lin[:1].copy()), None, 1, None,
                                                     1, 5, hp(np.empty((6, 1, 1))), hp(np.empty((6, 1, 1, 1))), None, None, None))):
        with pytest.raises(_lib.GPKError, match="finalised") as ei:
            raw._backend().call(entry, *args)
        assert ei.value.code == _lib.GPK_BAD_ARG
    # batched mode, and option small_path = 0: the library refuses, the Python layer says why
    be.call("gpk_batch_begin", 2)
    try:
        for call in (query, chain):
            with pytest.raises(_lib.GPKError, match="batched mode"):
                call()
    finally:
        be.call("gpk_batch_end")
    be.set_options(small_path=0)
    try:
        assert not bg.propagate_ok()
        for call in (query, chain):
            with pytest.raises(_lib.GPKError, match="small_path"):
                call()
        with pytest.raises(ValueError, match="small_path"):
            bg.predict_moments(Q1, S1, **scalers("batch2"))
        for route in ("chain", "host"):
            with pytest.raises(ValueError, match="small_path"):
                bg.propagate_moments(x1, U1, lin, route=route, **kw)
    finally:
        be.set_options(small_path=1)
    # the refused calls wrote nothing ...
    assert all((a == 7.0).all() for a in (traj, Sigma, mean, cov, xcov))
    # ... and left the handles serving: the same bits as before
    same_bits("batch2 after the refusals", bg.propagate_moments(x1, U1, lin, return_stages=True, **kw), first)
    same_moments("batch2 after the refusals", bg.predict_moments(Q1, S1, **scalers("batch2")), firstq)
    gp = served("single3")
    c3 = problem("single3")[0]
    one = gp.propagate_moments(c3["x0"][0], c3["U"], c3["lin"])
    sbe = gp._backend()
    sbe.set_options(small_path=0)
    try:
        with pytest.raises(ValueError, match="small_path"):
            gp.predict_moments(np.zeros((1, 4)), None)
        with pytest.raises(ValueError, match="small_path"):
            gp.propagate_moments(c3["x0"][0], c3["U"], c3["lin"])
    finally:
        sbe.set_options(small_path=1)
    x33, U33 = rollouts(c3["x0"][0], c3["U"], 33)
    with pytest.raises(ValueError, match="R must be in"):
        gp.propagate_moments(x33, U33, c3["lin"])
    same_bits("single3 after the refusals", gp.propagate_moments(c3["x0"][0], c3["U"], c3["lin"]), one)


# ---- 9. the control-loop wrappers take the chain -----------------------------------------------------------------------------------
def test_pretrained_gp_takes_the_moment_chain_on_a_file_of_sparse_models(model_dict):
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    from unmanned_aerial_vehicles_amd.trainer import GPTrainer, OUTPUT_NAMES
    from test_gpu_sparse_batch import pretrained
    d, rows = model_dict
    pt = pretrained(d)
    bg, names = pt._fused()
    assert isinstance(bg, BatchedSparseGP) and bg.propagate_ok()
    state, Ug, dt = rows[0, :6], np.ascontiguousarray(rows[:8, 6:].T), 0.02
    S0, Q = spd(6)
    be = bg._ensure()[0][0]
    be.call("gpk_timing", 1)
    try:
        assert _advance_launches(be) == 0
        X, Sig = pt.propagate_horizon(state, Ug, dt, Sigma0=1e-3 * S0, process_noise=1e-2 * Q, method="moment")
        assert _advance_launches(be) == 8, "one finishing launch per stage: the wrapper took the moment chain"
    finally:
        be.call("gpk_timing", 0)
    assert X.shape == (6, 9) and Sig.shape == (9, 6, 6)
    _, lin = nominal_rollouts(GPTrainer._nominal_dynamics, state, Ug, dt, 1)
    sys_ = [pt.scalers_y[n] for n in names]
    wt, wS = bg.propagate_moments(state, np.ascontiguousarray(Ug.T), lin, coord=[OUTPUT_NAMES.index(n) for n in names],
                                  in_scaler=pt.scalers_X[names[0]], Sigma0=1e-3 * S0, process_noise=1e-2 * Q, route="host",
                                  out_scaler=([float(np.ravel(s.mean_)[0]) for s in sys_], [float(np.ravel(s.scale_)[0]) for s in sys_]))
    check("sparse file, method = moment, against the host loop: X", X, wt[:, 0].T, 1e-10)
    check("sparse file, method = moment, against the host loop: Sigma", Sig, wS[:, 0], 1e-10)
    lX, lS = pt.propagate_horizon(state, Ug, dt, Sigma0=1e-3 * S0, process_noise=1e-2 * Q)
    assert not np.array_equal(lS, Sig), "the linearised horizon is another one"


def test_simple_quadrotor_gp_takes_the_moment_chain_with_a_sparse_model():
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SimpleQuadrotorGP, SparseGP, WhiteKernel
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    rng = np.random.default_rng(77)
    n, m, H = 300, 60, 5
    X = rng.standard_normal((n, 10))
    Y = 0.2 * np.sin(X @ rng.standard_normal((10, 6)) / 2.0) + 0.02 * rng.standard_normal((n, 6))
    sp = SparseGP(ConstantKernel(0.9) * RBF(2.5 + 0.1 * np.arange(10)) + WhiteKernel(0.02), X[:m] + 0.05 * rng.standard_normal((m, 10)),
                  alpha=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0)).fit(X[:200], Y[:200])
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = sp, True
    state, Ug, dt = 0.3 * rng.standard_normal(6), 0.3 * rng.standard_normal((4, H)), 0.1
    _, lin = nominal_rollouts(sq._nominal_dynamics, state, Ug, dt, 1)
    S0, Q = spd(6)
    be = sp._backend()
    sp._ensure()
    be.call("gpk_timing", 1)
    try:
        Xh, Sig = sq.propagate_horizon(state, Ug, dt, Sigma0=0.05 * S0, process_noise=Q, method="moment")
        assert _advance_launches(be) == H, "one finishing launch per stage: the wrapper took the moment chain"
    finally:
        be.call("gpk_timing", 0)
    assert Xh.shape == (6, H + 1) and Sig.shape == (H + 1, 6, 6) and sq.prediction_count == H
    wt, wS = sp.propagate_moments(state, np.ascontiguousarray(Ug.T), lin, Sigma0=0.05 * S0, process_noise=Q, route="host")
    check("propagate_horizon(method = moment) with a SparseGP against route = host: X", Xh, wt[:, 0].T, 1e-10)
    check("propagate_horizon(method = moment) with a SparseGP against route = host: Sigma", Sig, wS[:, 0], 1e-10)
    # the model takes rows: the wrapper's next horizon is served with the Q of all of them
    sp.partial_fit(X[200:], Y[200:])
    Xh2, Sig2 = sq.propagate_horizon(state, Ug, dt, Sigma0=0.05 * S0, process_noise=Q, method="moment")
    full = SparseGP(ConstantKernel(0.9) * RBF(2.5 + 0.1 * np.arange(10)) + WhiteKernel(0.02), sp.inducing_, alpha=1e-6,
                    y_mean=Y.mean(axis=0), y_std=Y.std(axis=0)).fit(X, Y)
    ft, fS = full.propagate_moments(state, np.ascontiguousarray(Ug.T), lin, Sigma0=0.05 * S0, process_noise=Q)
    assert not np.array_equal(Sig2, Sig)
    check("after partial_fit: X against a model fitted on all rows", Xh2, ft[:, 0].T)
    check("after partial_fit: Sigma against a model fitted on all rows", Sig2, fS[:, 0])
