"""The two MFMA shapes of the fp16 x 2 variance launch (k5_direct_kernel<AB, 1>: v_mfma_f32_32x32x16_f16; <AB, 2>:
v_mfma_f32_16x16x32_f16; handle option k5_mfma_shape) on the dense factors, references and bars of tests/test_k5_refs.py, through the
C ABI as in tests/test_gpu_k5_forms.py (whose operand cache and helpers are imported, not copied).

Cases (test_k5_refs.DIRECT_CASES): a (N 1100, M 1900: <1>, padded walk, ragged band), d (700, 300: <2> forced), g (2000, 100: <4>
forced, one tile column), h (1, 1, D 1), i (129, 129, D 16), and the block-scale case (768, 200).  Each runs under k5_mfma_shape 1
and 2, each twice, into NaN-filled outputs:
* e = max_m |S_gpu - S| / S <= bar (test_k5_refs.case_bar) for both shapes, and the two shapes agree within the bar;
* identical bits between the two runs of one shape;
* the GPKK5 line is the same for both shapes and equals the mirror (k5_direct_form); the GPKSHAPE line names the shape asked for;
* nothing is written behind row M.
Further: d and g on gpk_split2_rows_f64's operand (source NaN above the diagonal, destination pre-filled with 0xFF) give, at both
shapes, the bits they give on gpk_split2_rows' operand - no unwritten chunk is read; the packed step gpk_predict_mean_var_split2
returns, at both shapes, the plain entry's variances times y_std^2 bit for bit and one set of means; a value of k5_mfma_shape
outside 0 .. 2 behaves as 0.

The 16x16x32 form sums a column's squares over the same values in another order (16-row groups, four registers, two lane folds),
so the two shapes differ in rounding only.  Measured on an MI355X, e 32x32x16 / 16x16x32 / between the two / bar: a 1.72e-7 /
1.59e-7 / 6.2e-8 / 1.75e-6, d 1.78e-7 / 1.59e-7 / 8.4e-8 / 3.56e-6, g 1.56e-7 / 1.39e-7 / 8.3e-8 / 3.96e-6, h 9.49e-8 / 9.49e-8 / 0 /
3.40e-5, i 1.32e-7 / 1.33e-7 / 8.8e-8 / 3.37e-6, the block-scale case 3.36e-7 / 3.16e-7 / 1.24e-7 / 8.47e-6 (every case prints its
own); 61 440 / 491 520 chunks of d / g left as 0xFF by the fp64-source splitter, the same variance bits at both shapes."""
import numpy as np
import pytest

from test_gpu_k5_forms import _dp, _p, be, dev_case, f64_source, nan_bytes, nan_f64, s_err, split2_operand, split_f64  # noqa: F401
from test_k5_refs import DIRECT_CASES, SCALE_CASE, SF2, case_bar, case_operands, k5_direct_form, rel_err, scale_case_factor

pytestmark = pytest.mark.gpu

SHAPE_NAME = {1: "32x32x16", 2: "16x16x32"}
CASES = {name: DIRECT_CASES[name] for name in "adghi"}
CASES["scale"] = SCALE_CASE + (0,)


def lines(capfd, prefix):
    """The words behind `prefix` of the lines written to stderr since the last call that start with it, and the rest."""
    err = capfd.readouterr().err.splitlines()
    return [ln.split()[1:] for ln in err if ln.startswith(prefix + " ")], [ln for ln in err if not ln.startswith(prefix + " ")]


def want_line(Np, Mp, opt):
    ab, bh, per, per_pad, ntmT, nst, grid = k5_direct_form(Np, Mp, opt)
    return ["direct", f"rows{128 * ab}", f"ntmT{ntmT}", f"ntn{Mp // 128}", f"nst{nst}", f"pad{per_pad}", f"grid{grid}"]


def run_shape(be, capfd, c, opt, shape, W2, scales, runs=2):
    """gpk_predict_var_inv_split2 under k5_split2_tile = opt and k5_mfma_shape = shape, `runs` times into NaN buffers.  Returns
    (var[:M] as NumPy, the words of the GPKSHAPE line); the GPKK5 line is asserted against the mirror."""
    import torch
    N, M, D, Np, Mp = c["N"], c["M"], c["D"], c["Np"], c["Mp"]
    out, named = [], None
    be.check(be.lib.gpk_set_option(be.h, b"k5_split2_tile", opt))
    be.check(be.lib.gpk_set_option(be.h, b"k5_mfma_shape", shape))
    try:
        for _ in range(runs):
            work2, var = nan_bytes(be, Np * Mp * 4), nan_f64(be, Mp + 64)
            capfd.readouterr()
            be.bind_stream()
            be.check(be.lib.gpk_predict_var_inv_split2(be.h, _p(c["X"]), N, D, _dp(c["ls"]), SF2, _p(W2), _p(scales), Np, _p(c["Xq"]), M,
                                                       c["kss"], 0.0, _p(work2), _p(var)))
            be.sync()
            shp, rest = lines(capfd, "GPKSHAPE")
            k5 = [ln.split()[1:] for ln in rest if ln.startswith("GPKK5 ")]
            assert k5 == [want_line(Np, Mp, opt)], (k5, want_line(Np, Mp, opt))
            assert len(shp) == 1 and len(shp[0]) == 1, shp
            named = shp[0][0]
            assert bool(torch.isnan(var[M:]).all()), "nothing behind row M may be written"
            out.append(var[:M].cpu().numpy())
    finally:
        be.check(be.lib.gpk_set_option(be.h, b"k5_split2_tile", 0))
        be.check(be.lib.gpk_set_option(be.h, b"k5_mfma_shape", 0))
    for o in out[1:]:
        assert np.array_equal(out[0].view(np.uint64), o.view(np.uint64)), "two runs must give identical bits"
    return out[0], named


def case_on_device(be, name):
    N, M, D, opt = CASES[name]
    if name == "scale":
        c = dev_case(be, N, M, D, W32=scale_case_factor()[1], key="scales")
        bar = case_bar("direct", N, M, D, 0, True)[0]
    else:
        c = dev_case(be, N, M, D)
        bar = case_bar("direct", N, M, D)[0]
    return c, opt, bar


@pytest.mark.parametrize("name", list(CASES))
def test_both_shapes(be, capfd, name):
    c, opt, bar = case_on_device(be, name)
    W2, scales = split2_operand(be, c)
    v = {}
    for shape in (1, 2):
        v[shape], named = run_shape(be, capfd, c, opt, shape, W2, scales)
        assert named == SHAPE_NAME[shape]
    e1, e2 = s_err(c, v[1]), s_err(c, v[2])
    d = rel_err(c["kss"] - v[2], c["kss"] - v[1])
    print(f"shapes, case {name}: N {c['N']} M {c['M']} rows {128 * k5_direct_form(c['Np'], c['Mp'], opt)[0]}: e 32x32x16 {e1:.2e}, 16x16x32 {e2:.2e}, "
          f"between the two {d:.2e}, bar {bar:.2e}")
    assert e1 <= bar and e2 <= bar and d <= bar


@pytest.mark.parametrize("name", ["d", "g"])
def test_f64_source_operand_at_both_shapes(be, capfd, name):
    """The launch on gpk_split2_rows_f64's operand - chunks right of the diagonal tile never written, still 0xFF - against the
    launch on gpk_split2_rows' operand: the same bits, so no unwritten chunk is read."""
    c, opt, _ = case_on_device(be, name)
    Np = c["Np"]
    W2, scales = split2_operand(be, c)
    dst, sc = split_f64(be, f64_source(be, case_operands(*CASES[name][:3])[3]), Np)
    left = int((dst.view(-1, 16) == 255).all(dim=1).sum())
    assert left == sum(128 * (Np // 16 - 8 * (rb // 4 + 1)) for rb in range(Np // 32)) > 0
    for shape in (1, 2):
        ref = run_shape(be, capfd, c, opt, shape, W2, scales, runs=1)[0]
        var, named = run_shape(be, capfd, c, opt, shape, dst, sc, runs=1)
        assert named == SHAPE_NAME[shape]
        assert np.array_equal(var.view(np.uint64), ref.view(np.uint64)), f"{named}: the launch must never read an unwritten chunk"
    print(f"fp64-source operand, case {name}: {left} chunks left as 0xFF, same variance bits at both shapes")


def test_shape_option_outside_its_range_is_the_default(be, capfd):
    c, opt, _ = case_on_device(be, "i")
    W2, scales = split2_operand(be, c)
    v0, named0 = run_shape(be, capfd, c, opt, 0, W2, scales, runs=1)
    assert named0 in SHAPE_NAME.values()
    for value in (3, -1, 16):
        v, named = run_shape(be, capfd, c, opt, value, W2, scales, runs=1)
        assert named == named0 and np.array_equal(v.view(np.uint64), v0.view(np.uint64)), value
    # ... and 0 is one of the two shapes, bit for bit
    shape0 = {n: s for s, n in SHAPE_NAME.items()}[named0]
    vs = run_shape(be, capfd, c, opt, shape0, W2, scales, runs=1)[0]
    assert np.array_equal(vs.view(np.uint64), v0.view(np.uint64))


def test_packed_step_at_both_shapes(be, capfd):
    """gpk_predict_mean_var_split2 on case d (256-row tiles forced): at each shape the variances of the plain entry at that shape
    times y_std^2, bit for bit, its GPKSHAPE line, and the same means at both."""
    import torch
    c, opt, _ = case_on_device(be, "d")
    N, M, D, Np, Mp = c["N"], c["M"], c["D"], c["Np"], c["Mp"]
    P, GUARD = 2, 64
    W2, scales = split2_operand(be, c)
    rng = np.random.default_rng(5)
    alpha = be.upload(rng.standard_normal((N, P)), torch.float32)
    ym, ys = rng.standard_normal(P), 0.5 + rng.random(P)
    means = {}
    for shape in (1, 2):
        var = run_shape(be, capfd, c, opt, shape, W2, scales, runs=1)[0]
        out = nan_f64(be, M * 2 * P + GUARD)
        tmp = torch.full((M * P,), float("nan"), dtype=torch.float32, device=be.device)
        work2 = nan_bytes(be, Np * Mp * 4)
        be.check(be.lib.gpk_set_option(be.h, b"k5_split2_tile", opt))
        be.check(be.lib.gpk_set_option(be.h, b"k5_mfma_shape", shape))
        try:
            capfd.readouterr()
            be.bind_stream()
            be.check(be.lib.gpk_predict_mean_var_split2(be.h, _p(c["X"]), _p(alpha), N, D, P, _dp(c["ls"]), SF2, None, _dp(ym), _dp(ys), _p(W2),
                                                        _p(scales), Np, _p(c["Xq"]), M, c["kss"], 0.0, _p(work2), _p(tmp), 0.0, None, _p(out)))
            be.sync()
        finally:
            be.check(be.lib.gpk_set_option(be.h, b"k5_split2_tile", 0))
            be.check(be.lib.gpk_set_option(be.h, b"k5_mfma_shape", 0))
        shp, rest = lines(capfd, "GPKSHAPE")
        assert shp == [[SHAPE_NAME[shape]]] and [ln.split()[1:] for ln in rest if ln.startswith("GPKK5 ")] == [want_line(Np, Mp, opt)]
        got = out.cpu().numpy()
        assert np.isnan(got[M * 2 * P:]).all(), "the guard band behind row M must stay untouched"
        got = got[:M * 2 * P].reshape(M, 2 * P)
        assert np.array_equal(got[:, P:], (var[:, None] * ys[None, :]) * ys[None, :]), "var * y_std^2 of the plain entry, bit for bit"
        means[shape] = got[:, :P]
    assert np.all(np.isfinite(means[1])) and np.array_equal(means[1], means[2])
