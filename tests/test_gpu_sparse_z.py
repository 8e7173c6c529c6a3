"""Training the inducing inputs of the sparse GP ("training Z") on the GPU against tests/golden/sparse_z_ref.npz
(NumPy / SciPy, two independent forms of every gradient): the column pass alone (`gpk_sparse_zgrad_pass`, epilogue 5 of the tile
GEMM) on every tile form of the row pass's table, the evaluation (`SparseGP.log_bound(..., eval_inducing_gradient=True)`,
`gpk_sparse_eval_z`) and `SparseGP.train(train_inducing=True)`.  Buffers start out as NaN (conftest: GPK_DEBUG_FILL).

The column pass's reference is the writer's `zpass_sums` (every term formed as the library forms it, by differences of the divided
coordinates), evaluated over row chunks whose sums are added: N m D terms would not fit in memory at the larger shapes.  Its own
error is that of adding at most 22 000 fp64 terms per entry, row after row within a chunk: below 1e-14 of the sum of their absolute
values, two orders under the bars."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN, relerr
from test_gemm_epilogue_refs import gemm_form, row_pass_launches
from test_gpu_gemm_epilogues import FORCE_128, ROW_CASES, gemm_lines, row_inputs, small_tiles_of
from test_gpu_sparse_train import FP64_BAR, LIMIT_BAR, ROUTE_BAR, case_a_kernel, case_a_model, run_pass, training_model
from test_sparse_train_host import load_writer
from test_sparse_z_host import load_z_writer

pytestmark = pytest.mark.gpu

W = 17      # doubles per inducing input in the column pass's result


@pytest.fixture(scope="module")
def ref():
    d = np.load(os.path.join(GOLDEN, "sparse_train_ref.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def zref():
    d = np.load(os.path.join(GOLDEN, "sparse_z_ref.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def writer():
    return load_writer()


@pytest.fixture(scope="module")
def zwriter():
    return load_z_writer()


def run_zpass(be, X, Yn, Z, ls, sf2, Cfull):
    """gpk_sparse_zgrad_pass on host arrays; Cfull ((m + P) x m) goes into the padded, zero-filled device layout.  Returns R
    (mp x 17), which starts out as NaN."""
    import torch
    n, D, m, P = X.shape[0], X.shape[1], Z.shape[0], Yn.shape[1]
    mp = (m + 127) // 128 * 128
    Cm = np.zeros((mp + 128, mp))
    Cm[:m, :m] = Cfull[:m]
    Cm[mp:mp + P, :m] = Cfull[m:]
    dX, dY, dZ, dC = be.upload(X), be.upload(Yn), be.upload(Z), be.upload(Cm)
    R = torch.full((mp, W), float("nan"), dtype=torch.float64, device=be.device)
    ls = np.ascontiguousarray(ls, dtype=np.float64)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with be.lock:
        be.bind_stream()
        be.check(be.lib.gpk_sparse_zgrad_pass(be.h, p(dX), p(dY), n, p(dZ), m, D, P, ls.ctypes.data_as(C.POINTER(C.c_double)),
                                              float(sf2), p(dC), mp, p(R)))
        be.sync()
    return R.cpu().numpy()


_zpass_ref = {}


def zpass_reference(zwriter, key, X, Yn, Z, ls, sf2, Cr):
    """(R, sums of absolute values), both (m, D + 1), over row chunks of about 32 MB of terms; once per shape."""
    if key not in _zpass_ref:
        n, D, m = X.shape[0], X.shape[1], Z.shape[0]
        chunk = max(1, int(4e6) // (m * D))
        R, Ra = np.zeros((m, D + 1)), np.zeros((m, D + 1))
        for r0 in range(0, n, chunk):
            r, ra = zwriter.zpass_sums(X[r0:r0 + chunk], Yn[r0:r0 + chunk], Z, ls, sf2, Cr)
            R += r
            Ra += ra
        _zpass_ref[key] = (R, Ra)
    return _zpass_ref[key]


def zpass_error(got, want, scale):
    """The largest error of an entry, of that entry's sum of absolute values; rows >= m and columns D .. 15 must be zero."""
    m, D = want.shape[0], want.shape[1] - 1
    idx = list(range(D)) + [16]
    assert np.isfinite(got).all(), "every entry of R is written (the buffer starts as NaN)"
    assert not got[m:].any(), "rows i >= m are exactly zero"
    assert not got[:, D:16].any(), "columns D .. 15 are exactly zero"
    return float(np.max(np.abs(got[:m][:, idx] - want) / scale))


def case_a_inputs(ref, zref):
    Yn = (ref["A_Y"] - ref["A_y_mean"]) / ref["A_y_std"]
    return (ref["A_X"], Yn, ref["A_Z"], ref["A_ls"], float(ref["A_hyper"][0]), ref["A_C"]), zref["A_zpass"], zref["A_zpass_abs"]


# ---- 1. the column pass alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel", [256, 0])
def test_column_pass_case_a(ref, zref, panel):
    """panel = 256: three panels, the last with 188 rows."""
    from unmanned_aerial_vehicles_amd.device import Backend
    be = Backend(0).set_options(sparse_panel=panel)
    inputs, want, scale = case_a_inputs(ref, zref)
    runs = [run_zpass(be, *inputs) for _ in range(2)]
    e = zpass_error(runs[0], want, scale)
    print(f"panel {panel}: column pass against the fixture {e:.2e} of each entry's sum of absolute values")
    assert e < ROUTE_BAR
    assert np.array_equal(runs[0], runs[1]), "two runs must give identical bits"
    # column 16 over the inducing inputs is the row pass's unweighted sum
    sums = run_pass(be, *inputs)
    d = abs(runs[0][:, 16].sum() - sums[16]) / float(ref["A_pass_abs"][-1])
    print(f"panel {panel}: sum of column 16 against sums[16] of the row pass {d:.2e}")
    assert d < ROUTE_BAR
    be.lib.gpk_destroy(be.h)


@pytest.mark.parametrize("m,n,D,P", [(1, 17, 3, 2), (128, 17, 16, 16), (5, 1, 4, 1)])
def test_column_pass_at_the_limits(zwriter, m, n, D, P):
    from unmanned_aerial_vehicles_amd.device import Backend
    rng = np.random.default_rng(842 + m + n)
    X, Z, Yn = rng.standard_normal((n, D)), rng.standard_normal((m, D)), rng.standard_normal((n, P))
    ls = 3.0 * (1.0 + 0.05 * np.arange(D))
    Cr = rng.standard_normal((m + P, m))
    want, scale = zwriter.zpass_sums(X, Yn, Z, ls, 0.9, Cr)
    be = Backend(0)
    runs = [run_zpass(be, X, Yn, Z, ls, 0.9, Cr) for _ in range(2)]
    e = zpass_error(runs[0], want, scale)
    print(f"m {m} n {n} D {D} P {P}: {e:.2e}")
    assert e < (LIMIT_BAR if D == 16 and P == 16 else ROUTE_BAR)
    assert np.array_equal(runs[0], runs[1]), "two runs must give identical bits"
    be.lib.gpk_destroy(be.h)


def zpass_twice(opts, inputs, capfd):
    from unmanned_aerial_vehicles_amd.device import Backend
    be = Backend(0).set_options(gemm_log=1, **opts)
    gemm_lines(capfd)
    runs = [run_zpass(be, *inputs[:6]) for _ in range(2)]
    lines = gemm_lines(capfd)
    be.lib.gpk_destroy(be.h)
    return runs, lines


@pytest.mark.parametrize("name", list(ROW_CASES))
def test_column_pass_tile_forms(ref, zref, writer, zwriter, capfd, name):
    """Epilogue 5 on every tile form of the row pass's table: the form each case claims is computed from the launch rule and
    confirmed against the library's own `gemm_log` lines, as tests/test_gpu_gemm_epilogues.py does for epilogue 4."""
    opts, shape, bar, tile, tiles, direct = ROW_CASES[name]
    if shape is None:
        inputs, want, scale = case_a_inputs(ref, zref)
    else:
        inputs = row_inputs(ref, writer, shape)[:6]
        want, scale = zpass_reference(zwriter, shape, *inputs)
    X, Yn, Z = inputs[:3]
    n, D, m = X.shape[0], X.shape[1], Z.shape[0]
    launches = row_pass_launches(n, m, opts.get("sparse_panel", 0))
    forms = [gemm_form(rp, mp, small_tiles=small_tiles_of(opts)) for rp, mp, nt in launches]
    assert [f[0] for f in forms] == [tile] * len(tiles) and [f[1] for f in forms] == tiles and all(f[2] == direct for f in forms)
    rp, mp, nt = launches[0]
    runs, lines = zpass_twice(opts, inputs, capfd)
    assert lines == [(rp, mp, nt, 0, 1, 0) for rp, mp, nt in launches] * 2
    got = runs[0]
    e = zpass_error(got, want, scale)
    print(f"column pass {name}: n {n} m {m} D {D} P {Yn.shape[1]}: {len(launches)} panel(s) of {rp} x {mp}, {tile}-tiles, {tiles} tiles, "
          f"{'direct' if direct else 'super-tile walk'}: {e:.2e} of each entry's sum of absolute values")
    assert e < bar
    assert np.array_equal(runs[0], runs[1]), "two runs must give identical bits"
    if name.startswith(("c", "f")):
        # the 64-tile form of the same inputs: only the order of summation differs
        other, olines = zpass_twice({}, inputs, capfd)
        assert gemm_form(rp, mp)[0] == 64 and olines == lines
        idx = list(range(D)) + [16]
        d = float(np.max(np.abs(other[0][:m][:, idx] - got[:m][:, idx]) / scale))
        print(f"column pass {name}: 64-tiles against 128-tiles {d:.2e}")
        assert d < ROUTE_BAR and zpass_error(other[0], want, scale) < bar


# ---- 2. the evaluation -----------------------------------------------------------------------------------------------
def z_bar(agree):
    """The larger of 1e-8 and ten times the case's stored two-form agreement: the reference is only that certain."""
    return max(FP64_BAR, 10.0 * float(agree[0]))


@pytest.mark.parametrize("variant,iso", [("free", False), ("free", True), ("noise fixed", False), ("constant fixed", False)],
                         ids=["ard", "isotropic", "noise-fixed", "constant-fixed"])
def test_log_bound_inducing_gradient_case_a(ref, zref, variant, iso):
    kernel = case_a_kernel(ref, variant, iso)
    gp = case_a_model(ref, kernel).hold(ref["A_X"], ref["A_Y"])
    value0, grad0 = gp.log_bound(kernel.theta, eval_gradient=True)
    value, grad, gZ = gp.log_bound(kernel.theta, eval_gradient=True, eval_inducing_gradient=True)
    assert value == value0 and np.array_equal(grad, grad0), "the bound and theta's gradient are those of the call without Z"
    pre = "Aiso" if iso else "A"
    want, bar = zref[pre + "_gradZ"], z_bar(zref[pre + "_gradZ_agree"])
    e = relerr(gZ, want)
    print(f"{variant}, {'isotropic' if iso else 'ARD'}: dL/dZ {e:.2e} of its largest component (bar {bar:.1e})")
    assert gZ.shape == want.shape and e < bar
    # giving the same Z explicitly changes nothing; the value alone too
    v2, g2, gZ2 = gp.log_bound(kernel.theta, eval_gradient=True, inducing=ref["A_Z"], eval_inducing_gradient=True)
    assert v2 == value and np.array_equal(g2, grad) and np.array_equal(gZ2, gZ)
    assert gp.log_bound(kernel.theta, inducing=ref["A_Z"]) == value == gp.bound()
    assert np.array_equal(gp.inducing_, ref["A_Z"]) and gp.n_rows_ == 700


def test_log_bound_inducing_gradient_training_case(ref, zref):
    gp = training_model(ref).hold(ref["T_X"], ref["T_Y"][:, 0])
    theta = gp.kernel_.theta
    value0, grad0 = gp.log_bound(theta, eval_gradient=True)
    value, grad, gZ = gp.log_bound(theta, eval_gradient=True, eval_inducing_gradient=True)
    assert value == value0 and np.array_equal(grad, grad0)
    bar = z_bar(zref["T_gradZ_agree"])
    e = relerr(gZ, zref["T_gradZ"])
    print(f"training case, start (m = 64, jitter_uu = 1e-4): dL/dZ {e:.2e} of its largest component (bar {bar:.1e})")
    assert e < bar


def test_moved_inducing_inputs(ref, writer):
    from unmanned_aerial_vehicles_amd import SparseGP
    kernel = case_a_kernel(ref)
    X, Y = ref["A_X"], ref["A_Y"]
    gp = case_a_model(ref, kernel).hold(X, Y)
    Zm = ref["A_Z"] + 0.05 * np.cos(np.arange(ref["A_Z"].size)).reshape(ref["A_Z"].shape)
    value, grad, gZ = gp.log_bound(kernel.theta, eval_gradient=True, inducing=Zm, eval_inducing_gradient=True)
    sf2, noise, alpha, jit = ref["A_hyper"]
    Yn = (Y - ref["A_y_mean"]) / ref["A_y_std"]
    want = writer.bound_value(X, Yn, Zm, ref["A_ls"], sf2, noise, alpha, jit)
    print(f"Z moved by 0.05 cos(k): bound {value:.9f} against bound_value {want:.9f}: {abs(value - want) / abs(want):.2e}")
    assert abs(value - want) < FP64_BAR * abs(want)
    assert np.array_equal(gp.inducing_, Zm) and gp.inducing_ is not Zm
    Xq = np.random.default_rng(855).standard_normal((40, 4))
    mean, std = gp.predict(Xq, return_std=True)
    fresh = SparseGP(gp.kernel_, Zm, alpha=float(alpha), jitter_uu=float(jit), y_mean=ref["A_y_mean"], y_std=ref["A_y_std"]).fit(X, Y)
    fm, fs = fresh.predict(Xq, return_std=True)
    assert np.array_equal(mean, fm) and np.array_equal(std, fs), "the model left behind is a fresh fit at the moved Z, bit for bit"
    assert fresh.bound() == value
    # the statistics exported are those of the moved Z
    assert np.array_equal(gp.statistics()["G"], fresh.statistics()["G"])
    with pytest.raises(ValueError):
        gp.log_bound(kernel.theta, inducing=Zm[:-1])
    bad = Zm.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        gp.log_bound(kernel.theta, inducing=bad)
    with pytest.raises(ValueError):
        gp.log_bound(None, eval_inducing_gradient=True)


# ---- 3. train --------------------------------------------------------------------------------------------------------
def small_model(ref, zref, kernel=None, Z=None):
    from unmanned_aerial_vehicles_amd import RBF, ConstantKernel, SparseGP, WhiteKernel
    sf2, ls0, ls1, noise = ref["T_start"]
    jitter, jit = ref["T_hyper"]
    if kernel is None:
        kernel = ConstantKernel(sf2) * RBF([ls0, ls1]) + WhiteKernel(noise)
    return SparseGP(kernel, zref["Z16_Z"] if Z is None else Z, alpha=float(jitter), jitter_uu=float(jit), y_mean=ref["T_y_mean"],
                    y_std=ref["T_y_std"])


def test_train_inducing(ref, zref, writer):
    X, y = ref["T_X"], ref["T_Y"][:, 0]
    numpy_gap = float(zref["Z16_bound_z_opt"]) - float(zref["Z16_bound_theta_opt"])
    fixed_z = small_model(ref, zref).train(X, y)
    gp = small_model(ref, zref)
    assert gp.train(X, y, train_inducing=True) is gp
    print(f"m = 16: bound {float(zref['Z16_bound_start']):.3f} at the start; trained kernel {fixed_z.bound_value_:.6f}, kernel and Z "
          f"{gp.bound_value_:.6f} (NumPy / SciPy: {float(zref['Z16_bound_theta_opt']):.6f}, {float(zref['Z16_bound_z_opt']):.6f})")
    assert np.array_equal(fixed_z.inducing_, zref["Z16_Z"]), "train_inducing=False leaves Z alone"
    assert gp.bound_value_ - fixed_z.bound_value_ > 0.5 * numpy_gap
    assert gp.inducing_.shape == (16, 2) and not np.array_equal(gp.inducing_, zref["Z16_Z"])
    assert np.array_equal(gp.kernel.theta, np.log(ref["T_start"])), "the kernel passed in is left alone"
    # bound_value_ is the writer's bound at what train returned
    comp = gp.kernel_.components()
    jitter, jit = ref["T_hyper"]
    Yn = (ref["T_Y"] - ref["T_y_mean"]) / ref["T_y_std"]
    want = writer.bound_value(X, Yn, gp.inducing_, np.asarray(comp.ls, dtype=np.float64), comp.sf2, comp.noise, jitter, jit)
    print(f"bound_value_ against bound_value at (kernel_, inducing_): {abs(gp.bound_value_ - want) / abs(want):.2e}")
    assert abs(gp.bound_value_ - want) < FP64_BAR * abs(want)
    assert gp.bound() == gp.bound_value_ and gp.n_rows_ == 600
    # the model left behind is the one a fresh object builds from the trained kernel and the trained Z
    Xq = np.random.default_rng(843).uniform(-3.0, 3.0, (40, 2))
    mean, std = gp.predict(Xq, return_std=True)
    fresh = small_model(ref, zref, gp.kernel_, gp.inducing_).fit(X, y)
    fm, fs = fresh.predict(Xq, return_std=True)
    assert mean.shape == (40,) and np.array_equal(mean, fm) and np.array_equal(std, fs)
    # pickle keeps the trained Z, the kernel and the predictions
    gp2 = pickle.loads(pickle.dumps(gp))
    assert np.array_equal(gp2.inducing_, gp.inducing_) and np.array_equal(gp2.kernel_.theta, gp.kernel_.theta)
    assert gp2.bound_value_ == gp.bound_value_
    pm, ps = gp2.predict(Xq, return_std=True)
    assert np.array_equal(pm, mean) and np.array_equal(ps, std)


def test_train_without_inducing_is_unchanged(ref):
    """The default reproduces the existing fixture's optimum, as tests/test_gpu_sparse_train.py::test_train has it."""
    X, y = ref["T_X"], ref["T_Y"][:, 0]
    gp = training_model(ref).train(X, y, train_inducing=False)
    opt = float(ref["T_bound_opt"])
    assert gp.bound_value_ >= opt - 1e-6 * abs(opt)
    assert np.array_equal(gp.inducing_, ref["T_Z"])
    again = training_model(ref).train(X, y)
    assert again.bound_value_ == gp.bound_value_ and np.array_equal(again.kernel_.theta, gp.kernel_.theta)
