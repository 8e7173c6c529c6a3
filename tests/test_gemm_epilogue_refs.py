"""The references of tests/test_gpu_gemm_epilogues.py, checked here without a GPU: the row pass of the sparse bound's gradient
evaluated in row chunks (the definition of tests/golden/make_golden_sparse_train.py::pass_sums; the (n, m, D) array of the largest
case does not fit at once) against tests/golden/sparse_train_ref.npz, `oracle.gp_oracle.predict_cov` against scikit-learn's
recorded covariance (tests/golden/cov_ref.npz), and the launch rules the GPU module asserts its tile forms with - a restatement
of gpk_gemm_tile / launch<> (gpk_gemm.hip) and of sparse_panel_for / sparse_slabs_for (gpk_sparse.hip) - against the figures
DESIGN.md and the README quote.  NumPy / SciPy only."""
import os

import numpy as np

from conftest import GOLDEN
from test_sparse_train_host import load_writer

SMALL_TILES = 1024    # the library's defaults: gemm_small_tiles, gemm_tiny_tiles
TINY_TILES = 320


# ---- the references -------------------------------------------------------------------------------------------------
def pass_sums_chunked(writer, X, Yn, Z, ls, sf2, Cm, chunk=None):
    """The row pass as `writer.pass_sums` defines it, evaluated over row chunks: the D per-feature sums and the unweighted one,
    and the sums of the absolute values of the same terms.  Every term is formed as the writer forms it (exact differences of
    the divided coordinates, Q = [Kfu | Yn] @ Cm), and the per-feature terms are added in the writer's order too - NumPy adds
    the (rows * m, D) terms row after row, and a chunk's sum starts from the running sums instead of zero - so the result does
    not depend on the chunk beyond the last bit or two.  (Adding per-chunk sums instead is as good a reference - both are
    within 2e-16 of the extended-precision sums, of the sum of absolute values - but the fixture's own sums of absolute
    values, 91 000 positive terms added in that order, are 1.9e-14 from the exact ones and only the same order reproduces
    them.)"""
    n, D, m = X.shape[0], X.shape[1], Z.shape[0]
    if chunk is None:
        chunk = max(1, int(4e6) // (m * D))          # the (chunk, m, D) arrays stay near 32 MB
    run, arun, un, aun = None, None, 0.0, 0.0
    for r0 in range(0, n, chunk):
        Kfu = writer.rbf(X[r0:r0 + chunk], Z, ls, sf2)
        T = (np.hstack([Kfu, Yn[r0:r0 + chunk]]) @ Cm) * Kfu
        W = (T[:, :, None] * writer.sqdiff(X[r0:r0 + chunk], Z, ls)).reshape(-1, D)
        run = W.sum(axis=0) if run is None else np.concatenate([run[None, :], W]).sum(axis=0)
        arun = np.abs(W).sum(axis=0) if arun is None else np.concatenate([arun[None, :], np.abs(W)]).sum(axis=0)
        un += T.sum()
        aun += np.abs(T).sum()
    return np.concatenate([run, [un]]), np.concatenate([arun, [aun]])


# ---- the launch rules -------------------------------------------------------------------------------------------------
def gemm_form(m, n, lower=False, nbatch=1, epilogue=1, small_tiles=SMALL_TILES, tiny_tiles=TINY_TILES):
    """(tile edge, tiles per problem, mapped directly) of a tile-GEMM launch of m x n (multiples of 128) whose output aliases
    no operand: fewer than `tiny_tiles` 128-tiles and the plain store: 32; fewer than `small_tiles`: 64; else 128 (the explicit
    batch counts: what matters is the launch's workgroups).  At most 512 tiles per problem map workgroups to tiles directly,
    more walk the grid in super-tiles."""
    assert m % 128 == 0 and n % 128 == 0
    t128 = (m // 128) * (m // 128 + 1) // 2 if lower else (m // 128) * (n // 128)
    t128 *= nbatch
    tile = 32 if (epilogue == 0 and t128 < tiny_tiles) else 64 if t128 < small_tiles else 128
    ntm, ntn = m // tile, n // tile
    tiles = ntm * (ntm + 1) // 2 if lower else ntm * ntn
    return tile, tiles, tiles <= 512


def rect_super_rows(ntm, ntn):
    """Tile rows per band of the rectangle walk: 8; halved while the grid is shorter; widened for fewer than 8 tile columns."""
    sr = 8
    while sr > ntm:
        sr >>= 1
    if ntn < 8:
        sr = 8
        while 64 // sr > ntn and sr < 64:
            sr <<= 1
    return sr


def sparse_panel_rows(mp, option=0):
    """Rows per panel of the statistics and row passes: F = rows x (mp + 128) doubles within 128 MiB, 1024 .. 16384, a multiple
    of 256; the option `sparse_panel` overrides."""
    if option > 0:
        return option
    rows = (128 << 20) // ((mp + 128) * 8) // 256 * 256
    return min(max(rows, 1024), 16384)


def sparse_slabs(mp, rows, option=0):
    """k-slabs of one panel's product F^T F: one from 256 lower 128-tiles on; else the fewest that bring the launch to 1024
    tiles, at most 16, never slabs of fewer than 512 rows.  Returns (slabs, rows per slab)."""
    T = mp // 128 + 1
    tiles = T * (T + 1) // 2
    if option > 0:
        s = min(option, 64)
    elif tiles >= 256:
        s = 1
    else:
        s = max(1, min((1024 + tiles - 1) // tiles, 16, rows // 512))
    return s, ((rows + s - 1) // s + 63) // 64 * 64


def row_pass_launches(n, m, panel_option=0):
    """[(rows_p, mp, nt)] of the row pass's tile GEMMs, one per panel."""
    mp = (m + 127) // 128 * 128
    panel = sparse_panel_rows(mp, panel_option)
    return [((min(panel, n - r0) + 127) // 128 * 128, mp, mp + 128) for r0 in range(0, n, panel)]


# ---- the checks -----------------------------------------------------------------------------------------------------
def test_chunked_row_pass_reproduces_the_fixture():
    d = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    w = load_writer()
    Yn = (d["A_Y"] - d["A_y_mean"]) / d["A_y_std"]
    for chunk in (1, 97, 256, None):                # row by row, eight ragged chunks, three, one
        sums, asums = pass_sums_chunked(w, d["A_X"], Yn, d["A_Z"], d["A_ls"], d["A_hyper"][0], d["A_C"], chunk)
        e = (np.max(np.abs(sums - d["A_pass"]) / d["A_pass_abs"]), np.max(np.abs(asums - d["A_pass_abs"]) / d["A_pass_abs"]))
        print(f"chunk {chunk}: sums {e[0]:.2e}, sums of absolute values {e[1]:.2e} of the sum of absolute values")
        assert sums.shape == (5,) and max(e) < 1e-14
    whole = w.pass_sums(d["A_X"], Yn, d["A_Z"], d["A_ls"], d["A_hyper"][0], d["A_C"])
    assert np.array_equal(whole[0], d["A_pass"]) and np.array_equal(whole[1], d["A_pass_abs"])


def test_chunked_row_pass_against_extended_precision():
    """The reference's own error, where the GPU module uses it: random inputs as test_row_pass_at_the_limits draws them, the
    terms formed in fp64 and added in np.longdouble.  The fp64 sums must stay two orders below the GPU tests' 1e-12."""
    w = load_writer()
    rng = np.random.default_rng(861)
    for n, m, D, P in ((3000, 200, 4, 2), (900, 260, 16, 16), (129, 129, 1, 1)):
        X, Z, Yn = rng.standard_normal((n, D)), rng.standard_normal((m, D)), rng.standard_normal((n, P))
        ls = 3.0 * (1.0 + 0.05 * np.arange(D))
        Cr = rng.standard_normal((m + P, m))
        sums, asums = pass_sums_chunked(w, X, Yn, Z, ls, 0.9, Cr, chunk=500)
        Kfu = w.rbf(X, Z, ls, 0.9)
        T = (np.hstack([Kfu, Yn]) @ Cr) * Kfu
        W = T[:, :, None] * w.sqdiff(X, Z, ls)
        want = np.concatenate([W.astype(np.longdouble).sum(axis=(0, 1)), [T.astype(np.longdouble).sum()]])
        e = float(np.max(np.abs(sums - want) / asums))
        print(f"n {n} m {m} D {D} P {P}: fp64 sums against extended-precision sums {e:.2e} of the sum of absolute values")
        assert e < 1e-14


def test_predict_cov_reproduces_sklearn(csv_data):
    """The model of test_gpu_cov.py::test_one_target_unnormalised_matches_sklearn: RBF(0.5) + WhiteKernel(0.1), alpha 1e-4, one
    target, not normalised - fit_fixed reproduces it, so normalised units are the estimator's."""
    from oracle import gp_oracle as O
    ref = np.load(os.path.join(GOLDEN, "cov_ref.npz"))["one_cov"]
    st = O.fit_fixed(csv_data["X10"], csv_data["Y6"][:, 0], 0.5, 1.0, 0.1, 1e-4, normalize_y=False)
    cov = O.predict_cov(st, csv_data["Xq10"], 0.1)
    e = np.max(np.abs(cov - ref)) / np.max(np.abs(ref))
    print(f"predict_cov against scikit-learn: {e:.2e} of the largest entry")
    assert cov.shape == ref.shape == (64, 64) and e < 1e-10
    # a duplicated query: the prior without the noise off the diagonal, the same posterior reduction
    Xd = np.vstack([csv_data["Xq10"][:3], csv_data["Xq10"][:1]])
    cd = O.predict_cov(st, Xd, 0.1)
    assert abs(cd[0, 3] - (cd[0, 0] - 0.1)) < 1e-14 and abs(cd[3, 3] - cd[0, 0]) < 1e-14
    # ... and the diagonal is the variance path's
    _, std = O.predict(st, csv_data["Xq10"], return_std=True)
    assert np.max(np.abs(np.diag(cov) - std[:, 0] ** 2)) < 1e-13


def test_launch_rules_give_the_documented_figures():
    # the row pass at the sizes the README quotes: m = 1024 a 14 336-row panel, 896 128-tiles -> 3584 64-tiles, walked
    assert sparse_panel_rows(1024) == 14336 and gemm_form(14336, 1024) == (64, 3584, False)
    assert sparse_panel_rows(4096) == 3840 and (3840 // 128) * (4096 // 128) == 960
    assert sparse_panel_rows(16384) == 1024 and gemm_form(1024, 16384)[0] == 128
    assert sparse_panel_rows(256) == 16384
    # the statistics pass: m = 256 is 6 lower tiles, m = 1024 45, m = 4096 561 (one slab)
    assert sparse_slabs(256, 16384)[0] == 16 and sparse_slabs(1024, 14336)[0] == 16 and sparse_slabs(4096, 3840)[0] == 1
    assert sparse_slabs(256, 700) == (1, 704) and sparse_slabs(256, 256, 5) == (5, 64)
    # the covariance: the lower-triangle walk starts at 32 tile rows of 64, the 128-tile form at 1024 lower 128-tiles
    assert gemm_form(1920, 1920, lower=True) == (64, 465, True) and gemm_form(2048, 2048, lower=True) == (64, 528, False)
    assert gemm_form(5632, 5632, lower=True)[0] == 64 and gemm_form(5760, 5760, lower=True)[0] == 128
    # the plain store below gemm_tiny_tiles runs on 32-tiles whatever gemm_small_tiles says
    assert gemm_form(768, 768, lower=True, nbatch=6, epilogue=0, small_tiles=0)[0] == 32
    assert rect_super_rows(130, 4) == 16 and rect_super_rows(54, 10) == 8 and rect_super_rows(172, 3) == 32 and rect_super_rows(2, 2) == 32
    assert row_pass_launches(700, 130, 256) == [(256, 256, 384)] * 3 and row_pass_launches(22000, 300) == [(16384, 384, 512), (5632, 384, 512)]
