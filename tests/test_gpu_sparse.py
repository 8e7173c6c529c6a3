"""The sparse inducing-point GP on the GPU against tests/golden/sparse_ref.npz (NumPy / SciPy, two
independent forms): the statistics pass, the `SparseGP` class on cases A and B, determinism, the prior, the limits at their
smallest shapes, the refusals and the pickle round trip.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_sparse_host import dense_form

pytestmark = pytest.mark.gpu

ROUTE_BAR = 1e-12     # routes that differ in summation order only
FP64_BAR = 1e-8


@pytest.fixture(scope="module")
def ref():
    d = np.load(os.path.join(GOLDEN, "sparse_ref.npz"))
    return {k: d[k] for k in d.files}


def case_kernel(ref, case):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, WhiteKernel
    sf2, noise, alpha, jit = ref[case + "_hyper"]
    return ConstantKernel(sf2) * RBF(ref[case + "_ls"]) + WhiteKernel(noise), float(alpha), float(jit)


def case_a_model(ref):
    from unmanned_aerial_vehicles_amd import SparseGP
    kern, alpha, jit = case_kernel(ref, "A")
    return SparseGP(kern, ref["A_Z"], alpha=alpha, jitter_uu=jit, y_mean=ref["A_y_mean"], y_std=ref["A_y_std"])


def expected_std(ref, case):
    sf2, noise, alpha, jit = ref[case + "_hyper"]
    return np.sqrt(ref[case + "_var"] + noise)[:, None] * ref[case + "_y_std"][None, :]


# ---- 1. the statistics pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel,slabs", [(256, 0), (256, 1), (256, 5), (0, 0)])
def test_accumulate_case_a(ref, panel, slabs):
    import torch
    from unmanned_aerial_vehicles_amd.device import Backend
    be = Backend(0).set_options(sparse_panel=panel, sparse_slabs=slabs)
    X, Z, ls = ref["A_X"], ref["A_Z"], np.ascontiguousarray(ref["A_ls"])
    Yn = (ref["A_Y"] - ref["A_y_mean"]) / ref["A_y_std"]
    n, D, m, P = X.shape[0], X.shape[1], Z.shape[0], Yn.shape[1]
    mp = 256
    nt = mp + 128
    dX, dY, dZ = be.upload(X), be.upload(Yn), be.upload(Z)
    S = torch.zeros((nt, nt), dtype=torch.float64, device=be.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with be.lock:
        be.bind_stream()
        be.check(be.lib.gpk_sparse_accumulate(be.h, p(dX), p(dY), n, p(dZ), m, D, P, ls.ctypes.data_as(C.POINTER(C.c_double)),
                                              float(ref["A_hyper"][0]), p(S), nt))
        be.sync()
    assert torch.equal(S, S.T), "S must be symmetric bit for bit"
    S = S.cpu().numpy()
    G, g, yy = S[:m, :m], S[:m, mp:mp + P], np.diag(S)[mp:mp + P]
    e = (relerr(G, ref["A_G"]), relerr(g, ref["A_g"]), relerr(yy, ref["A_yy"]))
    print(f"panel {panel} slabs {slabs}: G {e[0]:.2e} g {e[1]:.2e} yy {e[2]:.2e}")
    assert max(e) < ROUTE_BAR
    assert np.isfinite(S).all()
    assert not S[m:mp].any() and not S[mp + P:].any(), "the padding of S must stay zero"
    be.lib.gpk_destroy(be.h)


# ---- 2. the class on case A ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pieces", [(700,), (300, 399, 1)])
def test_sparse_gp_case_a(ref, pieces):
    gp = case_a_model(ref)
    X, Y, Xq = ref["A_X"], ref["A_Y"], ref["A_Xq"]
    r0 = 0
    for k in pieces:
        gp.partial_fit(X[r0:r0 + k], Y[r0:r0 + k])
        r0 += k
    assert gp.n_rows_ == 700
    mean, std = gp.predict(Xq, return_std=True)          # 40 rows: the panel path
    e = (relerr(mean, ref["A_mean"]), relerr(std, expected_std(ref, "A")),
         abs(gp.bound() - float(ref["A_bound"])) / abs(float(ref["A_bound"])))
    print(f"pieces {pieces}: mean {e[0]:.2e} std {e[1]:.2e} bound {e[2]:.2e}")
    assert max(e) < FP64_BAR
    # the small path (slices of at most 32 rows) against the panel path
    parts = [gp.predict(Xq[a:b], return_std=True) for a, b in ((0, 32), (32, 40))]
    sm, ss = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    e2 = (relerr(sm, mean), relerr(ss, std))
    print(f"small against panel path: mean {e2[0]:.2e} std {e2[1]:.2e}")
    assert max(e2) < 1e-10
    assert max(relerr(sm, ref["A_mean"]), relerr(ss, expected_std(ref, "A"))) < FP64_BAR
    gp._backend().set_options(small_path=0)              # ... and the same slices through the panel path
    parts = [gp.predict(Xq[a:b], return_std=True) for a, b in ((0, 32), (32, 40))]
    gp._backend().set_options(small_path=1)
    pm, ps = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    assert max(relerr(pm, sm), relerr(ps, ss)) < 1e-10
    # means only
    assert relerr(gp.predict(Xq[:7]), sm[:7]) < ROUTE_BAR


# ---- 3. Z = X against the package's exact GP -------------------------------------------------------------------------
def test_case_b_against_exact_gp(ref):
    from unmanned_aerial_vehicles_amd import GaussianProcessRegressor, SparseGP
    kern, alpha, jit = case_kernel(ref, "B")
    X, y, Xq = ref["B_X"], ref["B_Y"][:, 0], ref["B_Xq"]
    exact = GaussianProcessRegressor(kernel=kern, alpha=alpha, normalize_y=True, optimizer=None).fit(X, y)
    em, es = exact.predict(Xq, return_std=True)
    sp = SparseGP.from_exact(exact, inducing=None, jitter_uu=jit).partial_fit(X, y)
    for rows in (slice(0, 40), slice(0, 25)):
        m_, s_ = sp.predict(Xq[rows], return_std=True)
        e = (relerr(m_, em[rows]), relerr(s_, es[rows]))
        print(f"rows {rows}: mean {e[0]:.2e} std {e[1]:.2e}")
        assert m_.shape == em[rows].shape and max(e) < FP64_BAR
    lml = exact.log_marginal_likelihood_value_
    eb = abs(sp.bound() - lml) / abs(lml)
    print(f"bound against the exact LML: {eb:.2e}")
    assert eb < FP64_BAR
    # an integer picks that many training rows, the same for the same seed
    z1 = SparseGP.from_exact(exact, inducing=50, random_state=3).inducing_
    z2 = SparseGP.from_exact(exact, inducing=50, random_state=3).inducing_
    assert z1.shape == (50, X.shape[1]) and np.array_equal(z1, z2)
    assert all((X == z).all(axis=1).any() for z in z1)


# ---- 4. determinism --------------------------------------------------------------------------------------------------
def test_same_updates_same_bits(ref):
    X, Y, Xq = ref["A_X"], ref["A_Y"], ref["A_Xq"]
    outs = []
    for _ in range(2):
        gp = case_a_model(ref)
        gp._backend().set_options(sparse_panel=256, sparse_slabs=3)
        gp.partial_fit(X[:450], Y[:450]).partial_fit(X[450:], Y[450:])
        st = gp.statistics()
        outs.append((st["G"], st["g"], st["yy"]) + gp.predict(Xq, return_std=True) + gp.predict(Xq[:25], return_std=True))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert np.array_equal(outs[0][0], outs[0][0].T)


# ---- 5. the prior, and one row ---------------------------------------------------------------------------------------
def test_prior_and_single_row(ref):
    from unmanned_aerial_vehicles_amd import SparseGP
    kern, alpha, jit = case_kernel(ref, "A")
    sf2, noise = ref["A_hyper"][:2]
    Z, Xq, ls = ref["A_Z"][:20], ref["A_Xq"], ref["A_ls"]
    ym, ys = np.array([0.7]), np.array([2.0])
    gp = SparseGP(kern, Z, alpha=alpha, jitter_uu=jit, y_mean=ym, y_std=ys)
    for rows in (slice(0, 40), slice(0, 5)):
        mean, std = gp.predict(Xq[rows], return_std=True)
        assert np.array_equal(mean, np.full(len(mean), 0.7))
        assert relerr(std ** 2, np.full(len(mean), (sf2 + noise) * 4.0)) < 1e-12
    assert gp.n_rows_ == 0 and gp.bound() == 0.0
    x1, y1 = ref["A_X"][:1], np.array([1.9])
    gp.partial_fit(x1, y1)
    mean_n, var, bound, _ = dense_form(x1, (y1[:, None] - ym) / ys, Z, Xq, ls, sf2, noise + alpha, jit)
    mean, std = gp.predict(Xq, return_std=True)
    e = (relerr(mean, ym + ys * mean_n[:, 0]), relerr(std, np.sqrt(var + noise) * 2.0), abs(gp.bound() - bound) / abs(bound))
    print(f"one row: mean {e[0]:.2e} std {e[1]:.2e} bound {e[2]:.2e}")
    assert max(e) < FP64_BAR and gp.n_rows_ == 1


# ---- 6. the limits at their smallest shapes --------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 1])
def test_smallest_shapes_at_the_limits(m):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    rng = np.random.default_rng(832 + m)
    N, D, P = 17, 16, 16
    X, Z, Xq = rng.standard_normal((N, D)), rng.standard_normal((m, D)), rng.standard_normal((33, D))
    if m == 1:
        Z = X[3:4] + 0.1
    Y = rng.standard_normal((N, P))
    ls = 3.0 * (1.0 + 0.05 * np.arange(D))
    sf2, noise, alpha = 0.9, 0.02, 1e-6
    ym, ys = Y.mean(axis=0), Y.std(axis=0)
    gp = SparseGP(ConstantKernel(sf2) * RBF(ls) + WhiteKernel(noise), Z, alpha=alpha, y_mean=ym, y_std=ys).fit(X, Y)
    mean_n, var, bound, _ = dense_form(X, (Y - ym) / ys, Z, Xq, ls, sf2, noise + alpha, 1e-8 * sf2)
    for rows in (slice(0, 33), slice(0, 9)):
        mean, std = gp.predict(Xq[rows], return_std=True)
        e = (relerr(mean, (ym + ys * mean_n)[rows]), relerr(std, (np.sqrt(var + noise)[:, None] * ys)[rows]))
        print(f"m {m} rows {rows}: mean {e[0]:.2e} std {e[1]:.2e}")
        assert mean.shape == (rows.stop, P) and max(e) < FP64_BAR
    assert abs(gp.bound() - bound) < FP64_BAR * abs(bound)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_errors(ref):
    from unmanned_aerial_vehicles_amd import RBF, SparseGP
    kern, alpha, jit = case_kernel(ref, "A")
    X, Y, Z = ref["A_X"], ref["A_Y"], ref["A_Z"]
    # (forty exact duplicates: each one's pivot is zero up to the sign of a rounding error, and one that is <= 0 is enough)
    dup = SparseGP(kern, np.concatenate([Z[:40], Z[:40]]), alpha=alpha, jitter_uu=0.0).partial_fit(X[:50], Y[:50])
    with pytest.raises(np.linalg.LinAlgError):
        dup.predict(X[:2])
    gp = case_a_model(ref).partial_fit(X[:60], Y[:60])
    with pytest.raises(ValueError):
        gp.partial_fit(X[:5, :3], Y[:5])
    with pytest.raises(ValueError):
        gp.partial_fit(X[:5], Y[:5, :1])
    bad = X[:5].copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        gp.partial_fit(bad, Y[:5])
    with pytest.raises(ValueError, match="P must be in"):
        SparseGP(kern, Z).partial_fit(X[:5], np.zeros((5, 17)))
    with pytest.raises(ValueError, match="NaN or infinity"):
        gp.predict(np.full((1, 4), np.inf))
    with pytest.raises(ValueError):
        gp.predict(X[:3, :2])
    with pytest.raises(ValueError):
        SparseGP(RBF(1.0) + RBF(2.0), Z)
    assert gp.n_rows_ == 60 and np.isfinite(gp.predict(X[:3])).all()      # the refusals left the model alone


# ---- 8. pickle -------------------------------------------------------------------------------------------------------
def test_pickle_round_trip(ref):
    gp = case_a_model(ref).partial_fit(ref["A_X"][:500], ref["A_Y"][:500])
    Xq = ref["A_Xq"]
    before = gp.predict(Xq, return_std=True) + gp.predict(Xq[:10], return_std=True)
    gp2 = pickle.loads(pickle.dumps(gp))
    assert gp2.n_rows_ == 500
    after = gp2.predict(Xq, return_std=True) + gp2.predict(Xq[:10], return_std=True)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert gp2.bound() == gp.bound()
    # the reloaded model goes on learning
    gp.partial_fit(ref["A_X"][500:], ref["A_Y"][500:])
    gp2.partial_fit(ref["A_X"][500:], ref["A_Y"][500:])
    assert relerr(gp2.predict(Xq), ref["A_mean"]) < FP64_BAR and np.array_equal(gp2.predict(Xq), gp.predict(Xq))
