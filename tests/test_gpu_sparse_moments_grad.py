"""The gradient through exact moment matching on the sparse posteriors (DESIGN.md, K11 "the gradient on the sparse models") on the
GPU: `SparseGP.predict_moments_vjp` / `propagate_moments_gradient` (`gpk_sparse_moments_vjp`, `gpk_sparse_propagate_mm_grad`), their
batch forms on `BatchedSparseGP` (`.._multi`), the taped sweep (five launches per stage forward, four backward) against the sweep
without the tape, and the control-loop wrappers.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL), so a stage that read another
stage's region of the tape, a slot no workgroup wrote or a row beyond m would show.

Expected values: `moments_vjp_numpy_form(sparse_form(name))` (tests/test_moments_grad_host.py on the form of
tests/test_sparse_moments_host.py).  Bar: the project's fp64 bar, 1e-8 of each array's largest component;
tests/test_sparse_moments_grad_host.py prints and asserts what it rests on, on these problems and horizons (float64 against
longdouble <= 2.9e-11; E[v] >= 1.8 % of the prior on every stage of 32 rollouts: the clip is inactive).  Bit identity is asserted with
np.array_equal.

Shapes: the problems of tests/test_sparse_propagate_host.py - single3 (m = 26, P = 3, D = 4: one tile, PC = 8), batch2 (B = 2, m = 60,
nx = 6, both scalers: a = b and a != b pairs, PC = 1), batch8 (36 pairs, a permuted coord, 14 query groups over 17 or 32 queries),
one200 (m = 200: 10 lower tiles, rows 200 .. 255 of Q masked) - with H = 4 and R = 1, 5, 17, 32."""
import sys

import numpy as np
import pytest

from test_gpu_paths import check
from test_gpu_sparse_batch import model_dict  # noqa: F401  (the fixture: six sparse models behind one input scaler)
from test_gpu_sparse_moments import backend_of, scalers
from test_gpu_sparse_propagate import _advance_launches, served
from test_moments_grad_host import horizon_seeds, moments_vjp_numpy_form, seeds
from test_propagate_host import rollouts, spd
from test_sparse_moments_grad_host import GPU_H, horizon_of
from test_sparse_moments_host import gaussian_rows, model_defs, sparse_form, sparse_moments_numpy_form
from test_sparse_propagate_host import PROBLEMS, problem

pytestmark = pytest.mark.gpu

NAMES = ("traj", "Sigma", "dU", "dx0", "dSigma0")


def check_grad(tag, got, want, tol=None):
    for what, g, w in zip(NAMES, got, want):
        check(f"{tag}: {what}", np.asarray(g), np.asarray(w), *(() if tol is None else (tol,)))


def same_grad(tag, a, b):
    for what, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), f"{tag}: {what}"


def tape_lines(capfd):
    """the GPKMT lines written to stderr since the last call, as dicts {tape, h, stage, launches}"""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    out = []
    for ln in cap.err.splitlines():
        assert not (ln.startswith("GPKMM ") and "tape" in ln)
        if ln.startswith("GPKMT "):
            w = ln.split()[1:]
            assert [x.rstrip("0123456789") for x in w] == ["tape", "h", "stage", "launches"], ln
            out.append({x.rstrip("0123456789"): int(x[len(x.rstrip("0123456789")):]) for x in w})
    return out


# ---- 1. parity with the NumPy adjoint ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (1, 5, 17, 32))
@pytest.mark.parametrize("name", PROBLEMS)
def test_predict_moments_vjp_parity(name, R):
    c = problem(name)[0]
    gp, mform = served(name), sparse_form(name)
    vform = moments_vjp_numpy_form(mform)
    nx, D = c["lin"].shape
    NO = mform.NO
    Q, S = gaussian_rows(name, R)
    gm, gc, gxc = seeds(R, NO, D)
    sc = scalers(name)
    for noisy in (False, True):
        got = gp.predict_moments_vjp(Q, S, gm, gc, gxc, var_includes_noise=noisy, **sc)
        assert got[3].shape == (R, D) and got[4].shape == (R, nx, nx)
        for a, b in zip(got[:3], gp.predict_moments(Q, S, var_includes_noise=noisy, **sc)):
            assert np.array_equal(a, b), "mean, cov and xcov have the bits of predict_moments"
        want = vform.batch(Q, S, noisy, gm, gc, gxc)
        check(f"{name}, R = {R}, noise {noisy}: dX", got[3], want[0])
        check(f"{name}, R = {R}, noise {noisy}: dSigma", got[4], want[1])
        assert np.array_equal(got[4], got[4].transpose(0, 2, 1)), "every dSigma equals its transpose bit for bit"
    # one seed at a time: None is zero; the seed of cov is symmetrised; no seed at all
    for k in range(3):
        one = [None] * 3
        one[k] = (gm, gc, gxc)[k]
        got = gp.predict_moments_vjp(Q, S, *one, **sc)
        want = vform.batch(Q, S, False, *one)
        check(f"{name}, R = {R}, seed {k} alone: dX", got[3], want[0])
        check(f"{name}, R = {R}, seed {k} alone: dSigma", got[4], want[1])
        zeros = [np.zeros_like(a) for a in (gm, gc, gxc)]
        zeros[k] = one[k]
        again = gp.predict_moments_vjp(Q, S, *zeros, **sc)
        assert np.array_equal(got[3], again[3]) and np.array_equal(got[4], again[4]), "a seed of None is a seed of zeros"
    sym = 0.5 * (gc + gc.transpose(0, 2, 1))
    a, b = gp.predict_moments_vjp(Q, S, None, gc, None, **sc), gp.predict_moments_vjp(Q, S, None, sym, None, **sc)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), "(g + g^T) / 2 is what is used"
    none = gp.predict_moments_vjp(Q, S, **sc)
    assert not none[3].any() and not none[4].any()


@pytest.mark.parametrize("name", ("single3", "batch2"))
def test_zero_and_rank_one_covariances_are_legal(name):
    gp, mform = served(name), sparse_form(name)
    Q, S = gaussian_rows(name, 5)
    S = 0.0 * S
    S[3] = np.outer(np.arange(1, S.shape[1] + 1), np.arange(1, S.shape[1] + 1)) * 1e-3      # rank one
    gm, gc, gxc = seeds(5, mform.NO, Q.shape[1])
    got = gp.predict_moments_vjp(Q, S, gm, gc, gxc, **scalers(name))
    want = moments_vjp_numpy_form(mform).batch(Q, S, False, gm, gc, gxc)
    check(f"{name}, Sigma = 0 and rank one: dX", got[3], want[0])
    check(f"{name}, Sigma = 0 and rank one: dSigma", got[4], want[1])


@pytest.mark.parametrize("R", (1, 5, 17, 32))
@pytest.mark.parametrize("name", PROBLEMS)
def test_propagate_moments_gradient_parity(name, R):
    c, _, kw, _ = problem(name)
    gp, mform = served(name), sparse_form(name)
    vform = moments_vjp_numpy_form(mform)
    lin, coord = c["lin"], model_defs(name)[3]
    nx = lin.shape[0]
    x0, U, S0, Q = horizon_of(name, R)
    H = U.shape[1]
    gx, gS = horizon_seeds(H, R, nx)
    for noisy, extra, want_args in ((True, dict(Sigma0=S0, process_noise=Q), (S0, Q)), (False, {}, (None, None))):
        got = gp.propagate_moments_gradient(x0, U, lin, gx, gS, var_includes_noise=noisy, **kw, **extra)
        assert got[2].shape == (R, H, U.shape[2]) and got[3].shape == (R, nx) and got[4].shape == (R, nx, nx)
        fwd = gp.propagate_moments(x0, U, lin, var_includes_noise=noisy, **kw, **extra)
        assert np.array_equal(got[0], fwd[0]) and np.array_equal(got[1], fwd[1]), "traj and Sigma have the bits of propagate_moments"
        check_grad(f"{name}, R = {R}, noise {noisy}", got, vform.horizon(coord, x0, U, lin, *want_args, gx, gS, noisy))
        assert np.array_equal(got[4], got[4].transpose(0, 2, 1))


# ---- 2. bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_repeatable_and_independent_of_batch_groups_and_tape(name):
    c, _, kw, _ = problem(name)
    gp = served(name)
    be = backend_of(gp)
    lin = c["lin"]
    nx = lin.shape[0]
    x0, U, S0, Q = horizon_of(name, 17)
    gx, gS = horizon_seeds(GPU_H, 17, nx)
    args = dict(Sigma0=S0, process_noise=Q, **kw)
    one = gp.propagate_moments_gradient(x0, U, lin, gx, gS, **args)
    same_grad(f"{name}: two calls", gp.propagate_moments_gradient(x0, U, lin, gx, gS, **args), one)
    for r in (0, 9, 16):
        alone = gp.propagate_moments_gradient(x0[r:r + 1], U[r:r + 1], lin, gx[:, r:r + 1], gS[:, r:r + 1], Sigma0=S0[r:r + 1],
                                              process_noise=Q, **kw)
        same_grad(f"{name}: rollout {r} of 17 against that rollout alone",
                  (one[0][:, r:r + 1], one[1][:, r:r + 1], one[2][r:r + 1], one[3][r:r + 1], one[4][r:r + 1]), alone)
    for groups in (1, 3):
        be.set_options(moments_query_groups=groups)
        try:
            same_grad(f"{name}: at most {groups} group(s) of queries", gp.propagate_moments_gradient(x0, U, lin, gx, gS, **args), one)
        finally:
            be.set_options(moments_query_groups=0)
    be.set_options(moments_tape_mb=0)
    try:
        same_grad(f"{name}: without the tape", gp.propagate_moments_gradient(x0, U, lin, gx, gS, **args), one)
    finally:
        be.set_options(moments_tape_mb=1024)


def test_the_budget_decides_the_sweep_and_changes_no_bit(capfd):
    """moments_tape_mb = 1: single3 at R = 1 (a stage of a few thousand doubles) is still taped, batch8 at R = 32 (64 slots of 32 x
    128 x 17 doubles of row vectors alone: 35 MB per stage) takes the 13 H sweep - read off the GPKMT line"""
    for name, R, small in (("single3", 1, True), ("batch8", 32, False)):
        c, _, kw, _ = problem(name)
        gp = served(name)
        be = backend_of(gp)
        lin = c["lin"]
        x0, U, S0, Q = horizon_of(name, R)
        gx, gS = horizon_seeds(GPU_H, R, lin.shape[0])
        args = dict(Sigma0=S0, process_noise=Q, **kw)
        gp.propagate_moments_gradient(x0, U, lin, gx, gS, **args)      # (the model is assembled, Q formed)
        got = {}
        be.set_options(gram_log=1)
        try:
            for mb in (1024, 1, 0):
                be.set_options(moments_tape_mb=mb)
                tape_lines(capfd)
                got[mb] = gp.propagate_moments_gradient(x0, U, lin, gx, gS, **args)
                lines = tape_lines(capfd)
                assert len(lines) == 1, (name, mb, lines)
                ln = lines[0]
                taped = mb == 1024 or (mb == 1 and small)
                assert ln["tape"] == int(taped) and ln["h"] == GPU_H and ln["launches"] == (9 if taped else 13) * GPU_H, (name, mb, ln)
                assert (ln["stage"] * 8 * GPU_H <= (mb << 20)) == taped, (name, mb, ln)
            tape_lines(capfd)
            gp.propagate_moments(x0, U, lin, **args)
            assert tape_lines(capfd) == [], "the forward chain does not ask for the tape"
        finally:
            be.set_options(gram_log=0, moments_tape_mb=1024)
        same_grad(f"{name}, R = {R}: 1 MiB against the default", got[1], got[1024])
        same_grad(f"{name}, R = {R}: no tape against the default", got[0], got[1024])


def test_one_model_batch_has_the_bits_of_the_single_model():
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    c = problem("one200")[0]
    gp = served("one200")
    bg = BatchedSparseGP([gp])
    x0, U, S0, Q = horizon_of("one200", 5)
    gx, gS = horizon_seeds(GPU_H, 5, 1)
    Qr, Sr = gaussian_rows("one200", 17)
    gm, gc, gxc = seeds(17, 1, Qr.shape[1])
    for noisy in (False, True):
        for a, b in zip(bg.predict_moments_vjp(Qr, Sr, gm, gc, gxc, var_includes_noise=noisy),
                        gp.predict_moments_vjp(Qr, Sr, gm, gc, gxc, var_includes_noise=noisy)):
            assert np.array_equal(a, b), f"B = 1 against the model's own call, noise {noisy}"
        args = dict(Sigma0=S0, process_noise=Q, var_includes_noise=noisy)
        same_grad(f"B = 1 against the model's own chain, noise {noisy}", bg.propagate_moments_gradient(x0, U, c["lin"], gx, gS, **args),
                  gp.propagate_moments_gradient(x0, U, c["lin"], gx, gS, **args))


# ---- 3. the host route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("single3", "batch2"))
def test_host_route(name):
    c, _, kw, _ = problem(name)
    gp = served(name)
    lin = c["lin"]
    x0, U, S0, Q = horizon_of(name, 5)
    gx, gS = horizon_seeds(GPU_H, 5, lin.shape[0])
    chain = gp.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q, **kw)
    host = gp.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q, route="host", **kw)
    check_grad(f"{name}: the host route against the chain", host, chain)


# ---- 4. Z = X: the sparse model is the exact one ---------------------------------------------------------------------------------
def test_inducing_inputs_at_the_rows_agree_with_the_exact_model():
    """Z = X and jitter_uu = 1e-10 (tests/test_gpu_sparse_moments.py has the reasoning): the two MODELS agree within the gap of their
    NumPy forms, printed; the tolerance is min(10 x that gap, 1e-8), the forward test's rule"""
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    from test_gpu_moments import problem as exact_problem
    c, gp, mform = exact_problem("b")
    sf2, noise, alpha = c["hyper"]
    jit = 1e-10
    sp = SparseGP(ConstantKernel(sf2) * RBF(c["ls"]) + WhiteKernel(noise), c["X"], alpha=alpha, jitter_uu=jit,
                  y_mean=c["Y"].mean(axis=0), y_std=c["Y"].std(axis=0)).fit(c["X"], c["Y"])
    sform = sparse_moments_numpy_form([dict(X=c["X"], Y=c["Y"], Z=c["X"], ls=c["ls"], sf2=sf2, noise=noise, alpha=alpha, jit=jit,
                                            ym=c["Y"].mean(axis=0), ys=c["Y"].std(axis=0))])
    lin = c["lin"]
    nx = lin.shape[0]
    S0, Q = spd(nx)
    x0, U = rollouts(c["x0"][0], c["U"][:GPU_H], 5)
    S0 = np.tile(0.05 * S0, (5, 1, 1))
    gx, gS = horizon_seeds(GPU_H, 5, nx)
    a = moments_vjp_numpy_form(sform).horizon(range(nx), x0, U, lin, S0, Q, gx, gS)
    b = moments_vjp_numpy_form(mform).horizon(range(nx), x0, U, lin, S0, Q, gx, gS)
    gap = max(float(np.max(np.abs(x - y)) / np.max(np.abs(y))) for x, y in zip(a, b))
    tol = min(10.0 * gap, 1e-8)
    print(f"Z = X: the two models' NumPy forms differ by {gap:.2e}; tolerance min(10 x that, 1e-8) = {tol:.2e}")
    got = sp.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q)
    want = gp.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q)
    check_grad("Z = X: SparseGP against GaussianProcessRegressor", got, want, tol)


# ---- 5. Q follows the model ---------------------------------------------------------------------------------------------------------
def test_the_gradient_follows_the_model_after_more_rows():
    from test_gpu_sparse_batch import ALPHA, build_model
    c = problem("one200")[0]
    p = c["ps"][0]
    first = dict(p, X=p["X"][:200], y=p["y"][:200])
    gp = build_model(first)
    lin = c["lin"]
    x0, U, S0, Q = horizon_of("one200", 5)
    gx, gS = horizon_seeds(GPU_H, 5, 1)

    def form(q):
        return sparse_moments_numpy_form([dict(X=q["X"], Y=q["y"][:, None], Z=q["Z"], ls=q["ls"], sf2=q["sf2"], noise=q["noise"],
                                               alpha=ALPHA, jit=1e-8 * q["sf2"], ym=np.array([q["ym"]]), ys=np.array([q["ys"]]))])

    before = gp.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q)
    check_grad("200 rows", before, moments_vjp_numpy_form(form(first)).horizon([0], x0, U, lin, S0, Q, gx, gS))
    gp.partial_fit(p["X"][200:], p["y"][200:])
    after = gp.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q)
    check_grad("300 rows: Q is that of all the rows", after,
               moments_vjp_numpy_form(sparse_form("one200")).horizon([0], x0, U, lin, S0, Q, gx, gS))
    assert not np.array_equal(before[2], after[2])


# ---- 6. a check that does not go through the NumPy adjoint ---------------------------------------------------------------------------
def test_directional_derivative_of_the_device_horizon():
    """<dU, delta U> against a central difference of l over two `propagate_moments` calls, by the step rule of the host file: 10 x
    the larger of the difference between steps h and h / 2 and eps |l| / h"""
    name = "batch2"
    c, _, kw, _ = problem(name)
    gp = served(name)
    lin = c["lin"]
    x0, U, S0, Q = horizon_of(name, 1)
    gx, gS = horizon_seeds(GPU_H, 1, lin.shape[0])
    dU = gp.propagate_moments_gradient(x0, U, lin, gx, gS, Sigma0=S0, process_noise=Q, **kw)[2]
    delta = np.random.default_rng(4).standard_normal(U.shape)

    def cost(t):
        traj, Sigma = gp.propagate_moments(x0, U + t * delta, lin, Sigma0=S0, process_noise=Q, **kw)
        return float(np.sum(gx * traj) + np.sum((gS + gS.transpose(0, 1, 3, 2)) / 2 * Sigma))

    h = 1e-4
    coarse, fine = (cost(h) - cost(-h)) / (2 * h), (cost(h / 2) - cost(-h / 2)) / h
    own = max(abs(coarse - fine), np.finfo(float).eps * abs(cost(0.0)) / h)
    err = abs(float(np.sum(dU * delta)) - fine)
    print(f"<dU, delta U> = {np.sum(dU * delta):.12e}, central difference {fine:.12e}: {err:.2e}; steps differ by "
          f"{abs(coarse - fine):.2e}, eps |l| / h = {np.finfo(float).eps * abs(cost(0.0)) / h:.2e}; asserted against 10 x {own:.2e}")
    assert err <= 10 * own


# ---- 7. refusals: nothing is written, the handles go on serving ---------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    import ctypes as C
    from unmanned_aerial_vehicles_amd import _lib
    from unmanned_aerial_vehicles_amd._lib import host_ptr as hp
    c, _, kw, _ = problem("batch2")
    bg = served("batch2")
    lin = c["lin"]
    x1, U1, S1h, Qn = horizon_of("batch2", 1)
    Q1, S1 = gaussian_rows("batch2", 1)
    gx, gS = horizon_seeds(GPU_H, 1, 6)
    gm, gc, gxc = seeds(1, 2, 10)
    first = bg.propagate_moments_gradient(x1, U1, lin, gx, gS, **kw)
    firstq = bg.predict_moments_vjp(Q1, S1, gm, gc, gxc, **scalers("batch2"))
    bes, good = bg._ensure()
    be = bes[0]
    H = GPU_H
    outs = dict(traj=np.full((H + 1, 1, 6), 7.0), Sigma=np.full((H + 1, 1, 6, 6), 7.0), dU=np.full((1, H, 4), 7.0), dx0=np.full((1, 6), 7.0),
                dS0=np.full((1, 6, 6), 7.0), mean=np.full((1, 2), 7.0), cov=np.full((1, 2, 2), 7.0), xcov=np.full((1, 2, 10), 7.0),
                dX=np.full((1, 10), 7.0), dS=np.full((1, 6, 6), 7.0))
    cd = (C.c_int * 2)(*c["coord"])
    U0 = np.ascontiguousarray(U1[0])
    D = {"dU": hp(outs["dU"]), "dx0": hp(outs["dx0"]), "dX": hp(outs["dX"]), "dS": hp(outs["dS"])}

    def chain(gx_=gx, gS_=gS, R=1, nx=6, **null):
        o = dict(D, **null)
        return be.call("gpk_sparse_propagate_mm_grad_multi", 2, good, 0, nx, cd, None, None, None, None, hp(x1), 1, hp(U0), 1, hp(lin),
                       None, 1, None, R, H, hp(outs["traj"]), hp(outs["Sigma"]), None, None, None, hp(gx_), hp(gS_), o["dU"], o["dx0"],
                       hp(outs["dS0"]))

    def query(gm_=gm, gc_=gc, gxc_=gxc, M=1, Xq=Q1, **null):
        o = dict(D, **null)
        return be.call("gpk_sparse_moments_vjp_multi", 2, good, 0, 6, None, None, None, None, hp(Xq), hp(S1), M, hp(outs["mean"]),
                       hp(outs["cov"]), hp(outs["xcov"]), hp(gm_), hp(gc_), hp(gxc_), o["dX"], o["dS"])

    nan_gx, inf_gS, nan_gm, inf_gc, nan_gxc, nanq = gx.copy(), gS.copy(), gm.copy(), gc.copy(), gxc.copy(), Q1.copy()
    nan_gx[2, 0, 1], inf_gS[H, 0, 5, 5], nan_gm[0, 1], inf_gc[0, 1, 0], nan_gxc[0, 0, 9], nanq[0, 3] = np.nan, np.inf, np.nan, np.inf, np.nan, np.nan
    for what, msg, call in (
            ("NaN in gx", "seeds gx and gS", lambda: chain(gx_=nan_gx)), ("infinity in gS", "seeds gx and gS", lambda: chain(gS_=inf_gS)),
            ("null gx", "null seed gx", lambda: chain(gx_=None)), ("null dx0", "null result dx0", lambda: chain(dx0=None)),
            ("null dU with controls", "null result dU", lambda: chain(dU=None)), ("R = 33", r"R must be in \[1, 32\]", lambda: chain(R=33)),
            ("nx below the number of outputs", "must not be below the number of outputs", lambda: chain(nx=1)),
            ("NaN in gmean", "seeds gmean, gcov and gxcov", lambda: query(gm_=nan_gm)),
            ("infinity in gcov", "seeds gmean, gcov and gxcov", lambda: query(gc_=inf_gc)),
            ("NaN in gxcov", "seeds gmean, gcov and gxcov", lambda: query(gxc_=nan_gxc)),
            ("null dXq", "null result dXq or dSq", lambda: query(dX=None)), ("null dSq", "null result dXq or dSq", lambda: query(dS=None)),
            ("M = 33", r"M must be in \[1, 32\]", lambda: query(M=33)), ("NaN in a query", "NaN or infinity", lambda: query(Xq=nanq))):
        with pytest.raises(_lib.GPKError, match=msg) as ei:
            call()
            pytest.fail(what)
        assert ei.value.code == _lib.GPK_BAD_ARG, what
    be.set_options(small_path=0)
    try:
        for call in (query, chain):
            with pytest.raises(_lib.GPKError, match="small_path"):
                call()
        with pytest.raises(ValueError, match="small_path"):
            bg.predict_moments_vjp(Q1, S1, gm, **scalers("batch2"))
        for route in ("chain", "host"):
            with pytest.raises(ValueError, match="small_path"):
                bg.propagate_moments_gradient(x1, U1, lin, gx, route=route, **kw)
    finally:
        be.set_options(small_path=1)
    assert all((a == 7.0).all() for a in outs.values()), "the refused calls wrote nothing"
    # a model without a finalised object behind its handle; then the same bits as before
    from test_gpu_sparse_batch import build_model, model_inputs
    raw = build_model(model_inputs(1, 60, 400, 10))
    with pytest.raises(_lib.GPKError, match="finalised"):
        raw._backend().call("gpk_sparse_moments_vjp", 0, 1, hp(Q1), None, 1, hp(outs["mean"]), hp(outs["cov"]), hp(outs["xcov"]), None, None,
                            None, hp(outs["dX"]), hp(outs["dS"]))
    assert all((a == 7.0).all() for a in outs.values())
    same_grad("batch2 after the refusals", bg.propagate_moments_gradient(x1, U1, lin, gx, gS, **kw), first)
    for a, b in zip(bg.predict_moments_vjp(Q1, S1, gm, gc, gxc, **scalers("batch2")), firstq):
        assert np.array_equal(a, b), "batch2 after the refusals: the query entry"
    # dSigma0 may be null
    chain_ok = be.call("gpk_sparse_propagate_mm_grad_multi", 2, good, 0, 6, cd, None, None, None, None, hp(x1), 1, hp(U0), 1, hp(lin),
                       None, 1, None, 1, H, hp(outs["traj"]), hp(outs["Sigma"]), None, None, None, hp(gx), hp(gS), hp(outs["dU"]),
                       hp(outs["dx0"]), None)
    assert chain_ok in (None, 0) and (outs["dS0"] == 7.0).all()
    plain = bg.propagate_moments_gradient(x1, U1, lin, gx, gS, coord=c["coord"])        # (no scalers, as the raw call)
    assert np.array_equal(outs["dU"], plain[2]) and np.array_equal(outs["dx0"], plain[3]) and np.array_equal(outs["traj"], plain[0])


# ---- 8. the control-loop wrappers take the chain -----------------------------------------------------------------------------------
def test_pretrained_gp_takes_the_gradient_chain_on_a_file_of_sparse_models(model_dict, capsys):
    from unmanned_aerial_vehicles_amd import BatchedSparseGP
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    from unmanned_aerial_vehicles_amd.trainer import GPTrainer, OUTPUT_NAMES
    from test_gpu_sparse_batch import pretrained
    d, rows = model_dict
    pt = pretrained(d)
    bg, names = pt._fused()
    assert isinstance(bg, BatchedSparseGP) and bg.propagate_ok()
    H = 4
    state, Ug, dt = rows[0, :6], np.ascontiguousarray(rows[:H, 6:].T), 0.02
    gx, gS = horizon_seeds(H, 1, 6)
    be = bg._ensure()[0][0]
    lin_before = pt.horizon_gradient(state, Ug, dt, gx[:, 0], gS[:, 0])
    capsys.readouterr()
    be.call("gpk_timing", 1)
    try:
        before = _advance_launches(be)
        got = pt.horizon_gradient(state, Ug, dt, gx[:, 0], gS[:, 0], method="moment")
        assert _advance_launches(be) - before == H, "one finishing launch per stage: the wrapper took the moment chain"
    finally:
        be.call("gpk_timing", 0)
    assert "failed" not in capsys.readouterr().out
    assert [a.shape for a in got] == [a.shape for a in lin_before]
    _, lin = nominal_rollouts(GPTrainer._nominal_dynamics, state, Ug, dt, 1)
    sys_ = [pt.scalers_y[n] for n in names]
    want = bg.propagate_moments_gradient(state, np.ascontiguousarray(Ug.T), lin, gx, gS, coord=[OUTPUT_NAMES.index(n) for n in names],
                                         in_scaler=pt.scalers_X[names[0]], route="host",
                                         out_scaler=([float(np.ravel(s.mean_)[0]) for s in sys_], [float(np.ravel(s.scale_)[0]) for s in sys_]))
    check("sparse file, method = moment, against the host route: X", got[0], want[0][:, 0].T)
    check("sparse file, method = moment, against the host route: dU", got[2], want[2][0])
    check("sparse file, method = moment, against the host route: dx0", got[3], want[3][0])
    again = pt.horizon_gradient(state, Ug, dt, gx[:, 0], gS[:, 0])
    assert all(np.array_equal(a, b) for a, b in zip(again, lin_before)), "without the keyword: the linear chain's bits"
    assert not np.array_equal(again[2], got[2]), "the gradient through the moments is another one"


def test_simple_quadrotor_gp_takes_the_gradient_chain_with_a_sparse_model(capsys):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SimpleQuadrotorGP, SparseGP, WhiteKernel
    from unmanned_aerial_vehicles_amd.paths import nominal_rollouts
    rng = np.random.default_rng(77)
    n, m, H = 300, 60, 4
    X = rng.standard_normal((n, 10))
    Y = 0.2 * np.sin(X @ rng.standard_normal((10, 6)) / 2.0) + 0.02 * rng.standard_normal((n, 6))
    sp = SparseGP(ConstantKernel(0.9) * RBF(2.5 + 0.1 * np.arange(10)) + WhiteKernel(0.02), X[:m] + 0.05 * rng.standard_normal((m, 10)),
                  alpha=1e-6, y_mean=Y.mean(axis=0), y_std=Y.std(axis=0)).fit(X[:200], Y[:200])
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = sp, True
    state, Ug, dt = 0.3 * rng.standard_normal(6), 0.3 * rng.standard_normal((4, H)), 0.1
    _, lin = nominal_rollouts(sq._nominal_dynamics, state, Ug, dt, 1)
    gx, gS = horizon_seeds(H, 1, 6)
    be = sp._backend()
    sp._ensure()
    lin_before = sq.horizon_gradient(state, Ug, dt, gx[:, 0], gS[:, 0])
    capsys.readouterr()
    be.call("gpk_timing", 1)
    try:
        before = _advance_launches(be)
        got = sq.horizon_gradient(state, Ug, dt, gx[:, 0], gS[:, 0], method="moment")
        assert _advance_launches(be) - before == H, "one finishing launch per stage: the wrapper took the moment chain"
    finally:
        be.call("gpk_timing", 0)
    assert "failed" not in capsys.readouterr().out
    assert [a.shape for a in got] == [a.shape for a in lin_before]
    want = sp.propagate_moments_gradient(state, np.ascontiguousarray(Ug.T), lin, gx, gS, route="host")
    check("horizon_gradient(method = moment) with a SparseGP against route = host: X", got[0], want[0][:, 0].T)
    check("horizon_gradient(method = moment) with a SparseGP against route = host: dU", got[2], want[2][0])
    check("horizon_gradient(method = moment) with a SparseGP against route = host: dx0", got[3], want[3][0])
    direct = sp.propagate_gradient(state, np.ascontiguousarray(Ug.T)[None], lin, gx, gS, route="chain")
    again = sq.horizon_gradient(state, Ug, dt, gx[:, 0], gS[:, 0])
    assert all(np.array_equal(a, b) for a, b in zip(again, lin_before))
    assert np.array_equal(again[2], direct[2][0]) and np.array_equal(again[3], direct[3][0]), "without the keyword: the linear chain"
