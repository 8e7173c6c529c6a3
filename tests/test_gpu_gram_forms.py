"""Every launch form of the RBF kernel-matrix family (gpk_gram.hip) called directly through the C ABI, against the plain fp64
references of tests/test_gram_refs.py:

A  gpk_gram, strip kernel (D <= 16): strips of 1, 2 and 8 column tiles on both sides of each size boundary, the partial last strip
   group (nt mod 8 in {2, 4, 6}), and the header comment's claim - the same tiles bit for bit whatever the strip length;
B  the streaming-store form (Np >= 16 384);                    C  the tile-per-workgroup kernel (D > 16, features in chunks of 16);
D  gpk_gram into a pitched view that starts 16 bytes into its allocation, and the fp32 pitch that is refused;
E  gpk_cross_gram_t in both argument orders, dense and pitched;  F  gpk_gram_rows slabs, dense and pitched;
G  the fp64 exp over its whole range (normal, gradual underflow, under the clamp) through gpk_gram and gpk_cross_gram_t;
H  the fragment-order fp16 x 2 cross panel of the variance launch, decoded, and that launch on an exactly known W;
I / J  the (D4, P4) and (D4, B4) instantiation grids of gpk_predict_mean and gpk_predict_mean_multi;   K  gpk_colsumsq.

A fresh handle with the option `gram_log` per module: every Gram and mean case asserts the form it claims (gram_form / mean_form)
against the library's own GPKGRAM / GPKMEAN line, so that a later change of a launch rule cannot silently empty the cases.  Every
output buffer starts as NaN.  Inputs unless a group says otherwise: standard normal rows (a case of N rows takes the leading N of
one draw per D), ls = 0.7 sqrt(D) (1 + 0.02 d), sf2 = 1.3, diag_add = 0.25.  Matrices above 3000 rows are compared on the device
in 1024-row panels.  Bars: fp64 1e-13 sf2, fp32 2e-6 sf2 (test_gram_fp64, test_gram_fp32, test_cross_gram_t); the reference's own
error against mpmath is at most 2.9e-16 sf2 (test_gram_refs.py).

Two findings predicted from reading the code:
* gpk_gram accepted ldk % 2 == 0 for fp32 although every store is 16 bytes: confirmed and fixed (it now requires % 4; group D).
* gpk_gram_rows' memsets of padding-only rows (`rows x ldk` elements, pitch columns included) cannot be reached: the argument
  check wants row0 a multiple of 128 and row0 + padded(nrows) <= Np < N + 128, so every slab it accepts has a data row in each
  128-row block, and a slab wholly past N is refused.  Group F asserts both (the refusal, and the guard untouched for every slab
  that is accepted); the library is unchanged there.

Measured on an MI355X, worst case per group (every case prints its own figure):
* fp64 entries, of sf2: strip forms 3.0e-16, streaming 3.4e-16, tile kernel 2.6e-16, gpk_cross_gram_t 2.6e-16 - the reference's own
  error; gpk_gram_rows against gpk_gram: 0 (identical bits) in both dtypes;
* fp32 entries, of sf2: strip forms 2.4e-7, streaming 2.0e-7, tile kernel 2.8e-7, gpk_cross_gram_t 2.6e-7, the split panel 1.9e-7;
* the fp64 exp: 0.576 x 2^-52 relative in the normal range (0.58 ulp at worst), 0.50 units of 2^-1074 below it, 1560 exact zeros
  under the clamp, through gpk_gram and gpk_cross_gram_t alike;
* the split panel: h0 and h1 equal fp16(x) and fp16(x - h0) of the cross kernel's entries in every one of the 36 cases (no entry
  differs); the variance launch on W = I: std within 8.2e-8;
* gpk_predict_mean: fp64 2.2e-15, fp32 6.8e-7 of the largest mean; gpk_predict_mean_multi against the per-model launch: fp64
  4.3e-15, fp32 1.2e-6; gpk_colsumsq: exact.
"""
import ctypes as C
import sys

import numpy as np
import pytest

from oracle import gp_oracle as O
from test_gram_refs import colsumsq_form, decode_split2_panel, exp_table, gram_form, mean_form, padded, rbf_panel

pytestmark = pytest.mark.gpu

SF2, DIAG = 1.3, 0.25
F64_BAR, F32_BAR = 1e-13, 2e-6
NMAX = 16257


@pytest.fixture(scope="module")
def be():
    from unmanned_aerial_vehicles_amd.device import Backend
    b = Backend(0).set_options(gram_log=1)
    yield b
    b.lib.gpk_destroy(b.h)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _dp(a):
    from unmanned_aerial_vehicles_amd import _lib
    return a.ctypes.data_as(_lib._dp)


def _code(dtype):
    from unmanned_aerial_vehicles_amd import _lib
    return _lib.GPK_F64 if dtype == "f64" else _lib.GPK_F32


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == "f64" else torch.float32


def log_lines(capfd, tag):
    """The words of the `tag` lines (option gram_log) written to stderr since the last call."""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)               # (what the test has printed so far stays in its report)
    return [ln.split()[1:] for ln in cap.err.splitlines() if ln.startswith(tag + " ")]


def ls_of(D):
    return 0.7 * np.sqrt(D) * (1.0 + 0.02 * np.arange(D))


_draws = {}


def inputs(be, dtype, D, N):
    """(X as the kernel gets it, the same values in fp64 for the reference) on the device: the leading N rows of the draw of D."""
    import torch
    if D not in _draws:
        X = np.random.default_rng(7000 + D).standard_normal((NMAX, D))
        x64 = be.upload(X)
        x32 = x64.to(torch.float32)
        _draws[D] = {"f64": (x64, x64), "f32": (x32, x32.double())}
    Xk, Xr = _draws[D][dtype]
    return Xk[:N].contiguous(), Xr[:N].contiguous()


def run_gram(be, dtype, Xk, D, ls=None, sf2=SF2, diag=DIAG, out=None, ldk=None):
    """gpk_gram into a fresh NaN (Np, Np) buffer (or the view `out` of pitch `ldk`); returns the (Np, Np) tensor."""
    N = Xk.shape[0]
    Np = padded(N)
    K = be.empty((Np, Np), _tdt(dtype)) if out is None else out
    ls = ls_of(D) if ls is None else ls
    be.bind_stream()
    be.check(be.lib.gpk_gram(be.h, _code(dtype), _p(Xk), N, D, _dp(np.ascontiguousarray(ls)), sf2, diag, _p(K), Np if ldk is None else ldk))
    return K


def assert_form(capfd, dtype, N, D):
    form = gram_form(N, D)
    lines = log_lines(capfd, "GPKGRAM")
    assert lines == [[dtype, str(N), str(padded(N)), str(D), form[0], f"gs{form[1]}", f"nt{form[2]}", f"grid{form[3]}"]], (lines, form)
    return form


def check_gram(K, Xr, dtype, D, ls=None, sf2=SF2, diag=DIAG):
    """Everything a Gram case asserts but the form: parity over the N x N block (1024-row panels, on the device), exact symmetry,
    the exact diagonal, the identity in the padding, no NaN inside Np x Np.  Returns the worst error in units of sf2."""
    import torch
    N, Np = Xr.shape[0], K.shape[0]
    tdt = _tdt(dtype)
    ls = ls_of(D) if ls is None else ls
    bar = F64_BAR if dtype == "f64" else F32_BAR
    worst, nans, asym = 0.0, 0, 0
    for r0 in range(0, N, 1024):
        r1 = min(N, r0 + 1024)
        blk = K[r0:r1, :N]
        nans += int(torch.isnan(K[r0:r1, :Np]).sum())
        asym += int((blk != K[:N, r0:r1].T).sum())
        diff = (blk.double() - rbf_panel(Xr[r0:r1], Xr, ls, sf2)).abs_()
        i = torch.arange(r0, r1, device=K.device)
        diff[i - r0, i] = 0.0                                                   # (the diagonal is asserted exactly below)
        worst = max(worst, float(diff.nan_to_num_(nan=float("inf")).max()) / sf2)
    print(f"gram {dtype} N {N} D {D}: worst entry {worst:.2e} of sf2, {asym} entries differ from their mirror, {nans} NaN")
    assert nans == 0, "NaN left inside the padded block"
    assert asym == 0, "the data block must be exactly symmetric"
    dval = torch.tensor(sf2, dtype=tdt) + torch.tensor(diag, dtype=tdt)         # T(sf2) + T(diag_add), in T
    assert torch.equal(K.diagonal()[:N].cpu(), dval.expand(N)), "the diagonal must be exactly sf2 + diag_add"
    if Np > N:
        want = torch.zeros((Np - N, Np), dtype=tdt, device=K.device)
        want[torch.arange(Np - N), torch.arange(N, Np)] = 1.0
        assert torch.equal(K[N:, :Np], want) and torch.equal(K[:N, N:Np], want[:, :N].T), "rows and columns >= N must be the identity"
    assert worst <= bar, (worst, bar)
    return worst


# ---- A. strip forms ---------------------------------------------------------------------------------------------------
SMALL_N = [1, 64, 65, 128, 129, 2816, 2817]
LARGE_N = [7808, 7809, 8064, 8192, 8320]
STRIP_CASES = ([(n, dt, d) for n in SMALL_N for dt in ("f64", "f32") for d in (1, 3, 9, 16)]
               + [(n, "f64", d) for n in LARGE_N for d in (1, 3, 9, 16)] + [(n, "f32", 16) for n in LARGE_N])
WANT_GS = {2816: 1, 2817: 2, 7808: 2, 7809: 8, 8064: 8, 8192: 8, 8320: 8}
WANT_NT = {7809: 124, 8064: 126, 8192: 128, 8320: 130}


@pytest.mark.parametrize("N,dtype,D", STRIP_CASES)
def test_gram_strip_forms(be, capfd, N, dtype, D):
    Xk, Xr = inputs(be, dtype, D, N)
    log_lines(capfd, "GPKGRAM")
    K = run_gram(be, dtype, Xk, D)
    kern, gs, nt, grid, streaming = assert_form(capfd, dtype, N, D)
    assert kern == "strip" and not streaming and gs == WANT_GS.get(N, 1) and nt == WANT_NT.get(N, nt)
    e = check_gram(K, Xr, dtype, D)
    print(f"gram strip {dtype} N {N} D {D}: gs {gs} nt {nt} grid {grid}: {e:.2e} of sf2")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("D", [1, 3, 9, 16])
def test_gram_strip_lengths_give_identical_bits(be, capfd, dtype, D):
    """gram_strip_kernel's header: "the tiles themselves are computed identically whatever the strip length: bit-identical K"."""
    import torch
    K = {}
    for N in (2816, 7808, 8192):
        log_lines(capfd, "GPKGRAM")
        K[N] = run_gram(be, dtype, inputs(be, dtype, D, N)[0], D)
        assert assert_form(capfd, dtype, N, D)[1] == {2816: 1, 7808: 2, 8192: 8}[N]
    assert torch.equal(K[2816], K[7808][:2816, :2816]) and torch.equal(K[2816], K[8192][:2816, :2816])
    # (N = 7808 is a multiple of 128: no padding inside the leading block of the larger matrix)
    assert torch.equal(K[7808], K[8192][:7808, :7808])


# ---- B. streaming stores ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gram_streaming_strip(be, capfd, dtype):
    import torch
    N, D = 16257, 16
    Xk, Xr = inputs(be, dtype, D, N)
    log_lines(capfd, "GPKGRAM")
    K = run_gram(be, dtype, Xk, D)
    kern, gs, nt, grid, streaming = assert_form(capfd, dtype, N, D)
    assert (kern, gs, nt, streaming) == ("strip", 8, 256, True)
    e = check_gram(K, Xr, dtype, D)
    print(f"gram streaming {dtype} N {N} D {D}: gs {gs} nt {nt} grid {grid}: {e:.2e} of sf2")
    K8 = run_gram(be, dtype, inputs(be, dtype, D, 8192)[0], D)
    assert not gram_form(8192, D)[4] and torch.equal(K8, K[:8192, :8192])


# ---- C. tile-per-workgroup kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("D", [17, 32, 33, 48, 64])
def test_gram_tile_kernel(be, capfd, dtype, D):
    import torch
    K = {}
    for N in (200, 1000):
        Xk, Xr = inputs(be, dtype, D, N)
        log_lines(capfd, "GPKGRAM")
        K[N] = run_gram(be, dtype, Xk, D)
        kern, gs, nt, grid, streaming = assert_form(capfd, dtype, N, D)
        assert kern == "sym" and grid == nt * (nt + 1) // 2 and not streaming
        e = check_gram(K[N], Xr, dtype, D)
        print(f"gram tile kernel {dtype} N {N} D {D}: {grid} tiles, {(D + 15) // 16} feature chunks: {e:.2e} of sf2")
    assert torch.equal(K[200][:200, :200], K[1000][:200, :200])


def test_gram_tile_kernel_streaming(be, capfd):
    N, D = 16257, 17
    Xk, Xr = inputs(be, "f32", D, N)
    log_lines(capfd, "GPKGRAM")
    K = run_gram(be, "f32", Xk, D)
    assert assert_form(capfd, "f32", N, D) == ("sym", 0, 256, 32896, True)
    e = check_gram(K, Xr, "f32", D)
    print(f"gram tile kernel streaming f32 N {N} D {D}: {e:.2e} of sf2")


# ---- D. pitch and offset ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [1000, 3000])
def test_gram_pitched_offset_view(be, capfd, dtype, N):
    import torch
    D = 9
    Np = padded(N)
    es, lead = (8, 2) if dtype == "f64" else (4, 4)                 # the view starts 16 bytes into the allocation
    ldk = Np + lead                                                  # fp64: Np + 2, fp32: Np + 4
    Xk, Xr = inputs(be, dtype, D, N)
    dense = run_gram(be, dtype, Xk, D)
    buf = torch.full((lead + Np * ldk + 64,), float("nan"), dtype=_tdt(dtype), device=be.device)
    view = buf[lead:lead + Np * ldk].view(Np, ldk)
    assert view.data_ptr() == buf.data_ptr() + 16 and lead * es == 16
    log_lines(capfd, "GPKGRAM")
    run_gram(be, dtype, Xk, D, out=view, ldk=ldk)
    assert assert_form(capfd, dtype, N, D)[1] == {1000: 1, 3000: 2}[N]
    assert torch.equal(view[:, :Np], dense), "the pitched result must be the dense one bit for bit"
    # ... and nothing else was written: the pitch columns, the bytes before the view, the tail
    assert int((~torch.isnan(buf)).sum()) == Np * Np and not bool(torch.isnan(view[:, :Np]).any())


def test_gram_fp32_refuses_a_pitch_that_breaks_the_16_byte_stores(be, capfd):
    import torch
    from unmanned_aerial_vehicles_amd import _lib
    N, D = 1000, 9
    Np = padded(N)
    Xk, _ = inputs(be, "f32", D, N)
    buf = torch.full((Np * (Np + 2),), float("nan"), dtype=torch.float32, device=be.device)
    log_lines(capfd, "GPKGRAM")
    be.bind_stream()
    rc = be.lib.gpk_gram(be.h, _lib.GPK_F32, _p(Xk), N, D, _dp(ls_of(D)), SF2, DIAG, _p(buf), Np + 2)
    be.sync()
    assert rc == _lib.GPK_BAD_ARG and log_lines(capfd, "GPKGRAM") == [] and bool(torch.isnan(buf).all())
    # fp64 keeps % 2 (two doubles per store); an odd pitch is refused there too
    b64 = torch.full((Np * (Np + 2),), float("nan"), dtype=torch.float64, device=be.device)
    X64, _ = inputs(be, "f64", D, N)
    assert be.lib.gpk_gram(be.h, _lib.GPK_F64, _p(X64), N, D, _dp(ls_of(D)), SF2, DIAG, _p(b64), Np + 1) == _lib.GPK_BAD_ARG
    be.check(be.lib.gpk_gram(be.h, _lib.GPK_F64, _p(X64), N, D, _dp(ls_of(D)), SF2, DIAG, _p(b64), Np + 2))
    assert int((~torch.isnan(b64)).sum()) == Np * Np


# ---- E. gpk_cross_gram_t ------------------------------------------------------------------------------------------------
CROSS_SHAPES = [(300, 50, 9), (1, 1, 1), (129, 130, 16), (1000, 257, 17), (700, 300, 64), (65, 513, 3)]
_cross_ref = {}


def cross_case(N, M, D):
    """(X, Xq, ls, fp64 reference (N, M), the same from the fp32-rounded inputs), evaluated once per shape."""
    if (N, M, D) not in _cross_ref:
        rng = np.random.default_rng(100 * N + M + D)
        X, Xq = rng.standard_normal((N, D)), rng.standard_normal((M, D))
        ls = ls_of(D)
        r32 = O.rbf_cross(X.astype(np.float32).astype(np.float64), Xq.astype(np.float32).astype(np.float64), ls, SF2)
        _cross_ref[(N, M, D)] = (X, Xq, ls, O.rbf_cross(X, Xq, ls, SF2), r32)
    return _cross_ref[(N, M, D)]


def run_cross(be, dtype, A, Bq, ls, sf2, pitch):
    """gpk_cross_gram_t with rows = A, columns = Bq into a NaN (padded rows, padded columns + pitch) buffer."""
    na, nb, D = A.shape[0], Bq.shape[0], A.shape[1]
    Ad, Bd = be.upload(A, _tdt(dtype)), be.upload(Bq, _tdt(dtype))
    out = be.empty((padded(na), padded(nb) + pitch), _tdt(dtype))
    be.bind_stream()
    be.check(be.lib.gpk_cross_gram_t(be.h, _code(dtype), _p(Ad), na, _p(Bd), nb, D, _dp(np.ascontiguousarray(ls)), sf2, _p(out), out.shape[1]))
    be.sync()
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N,M,D", CROSS_SHAPES)
def test_cross_gram_t_shapes_pitches_orders(be, dtype, N, M, D):
    import torch
    X, Xq, ls, r64, r32 = cross_case(N, M, D)
    ref = r64 if dtype == "f64" else r32
    bar = F64_BAR if dtype == "f64" else F32_BAR
    for order in ("training-major", "query-major"):
        A, Bq, want = (X, Xq, ref) if order == "training-major" else (Xq, X, ref.T)
        na, nb = A.shape[0], Bq.shape[0]
        for pitch in (0, 128):
            out = run_cross(be, dtype, A, Bq, ls, SF2, pitch)
            got = out.double().cpu().numpy()
            blk = got[:, :padded(nb)]
            e = np.max(np.abs(blk[:na, :nb] - want)) / SF2
            print(f"cross_gram_t {dtype} {order} ({na} x {nb}, D {D}) ldb = Mp + {pitch}: {e:.2e} of sf2")
            assert e <= bar
            assert not blk[na:].any() and not blk[:, nb:].any(), "exact zeros in the padding"
            assert np.isnan(got[:, padded(nb):]).all(), "the pitch columns must stay untouched"
            assert not np.isnan(blk).any()


# ---- F. gpk_gram_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("D", [9, 17])
def test_gram_rows_slabs_and_guard(be, dtype, D):
    import torch
    from unmanned_aerial_vehicles_amd import _lib
    N = 700
    Np = padded(N)
    Xk, Xr = inputs(be, dtype, D, N)
    full = run_gram(be, dtype, Xk, D)
    ls = ls_of(D)
    # the bar of test_gram_row_slabs: the fused kernel mirrors tiles, a slab computes every entry directly
    bar = 4 * np.finfo(np.float64).eps * SF2 if dtype == "f64" else F32_BAR * SF2
    for pitch in (0, 128):
        ldk = Np + pitch
        for row0, nrows in ((0, 300), (640, 128), (0, 700)):
            nrp = padded(nrows)
            slab = be.empty((nrp, ldk), _tdt(dtype))
            be.bind_stream()
            be.check(be.lib.gpk_gram_rows(be.h, _code(dtype), _p(Xk), N, D, _dp(ls), SF2, DIAG, row0, nrows, _p(slab), ldk))
            be.sync()
            e = float((slab[:, :Np].double() - full[row0:row0 + nrp].double()).abs().max())
            print(f"gram_rows {dtype} D {D} rows [{row0}, {row0 + nrp}) ldk = Np + {pitch}: {e / SF2:.2e} of sf2")
            assert e <= bar
            assert torch.equal(slab[:, :Np].diagonal(row0), full.diagonal()[row0:row0 + nrp])
            if row0 + nrp > N:          # rows >= N: the identity padding, exactly (tile rows 704 .. 767 hold nothing else)
                assert torch.equal(slab[N - row0:, :Np], full[N:row0 + nrp])
            assert bool(torch.isnan(slab[:, Np:]).all()), "the pitch columns must stay untouched"
        # a slab wholly past N does not exist: row0 is a multiple of 128 and row0 + padded(nrows) <= Np < N + 128
        slab = be.empty((128, ldk), _tdt(dtype))
        for row0 in (Np, Np + 128):
            rc = be.lib.gpk_gram_rows(be.h, _code(dtype), _p(Xk), N, D, _dp(ls), SF2, DIAG, row0, 1, _p(slab), ldk)
            assert rc == _lib.GPK_BAD_ARG
        be.sync()
        assert bool(torch.isnan(slab).all())


# ---- G. the fp64 exp over its whole range -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exp_case():
    rng = np.random.default_rng(64)
    i = np.concatenate([np.arange(2600), rng.choice(2600, 40, replace=False)])
    i = i[rng.permutation(i.size)]
    return i, exp_table(2599)


@pytest.mark.parametrize("entry", ["gram", "cross_gram_t"])
def test_exp_fp64_whole_range(be, capfd, exp_case, entry):
    """D = 1, ls = 1, sf2 = 1, X = i / 64: every difference, square and halving is exact, so entry (a, b) is
    gpk_exp_neg(-(i_a - i_b)^2 / 8192) and nothing else.  Normal range: relative error <= 2^-52 against the 40-digit value;
    below 2^-1022: within 2 units of the least subnormal; under the clamp at -800: exactly 0; duplicates: exactly 1."""
    idx, (hi, lo, cls) = exp_case
    N = idx.size
    X = (idx / 64.0).reshape(N, 1)
    one = np.ones(1)
    if entry == "gram":
        log_lines(capfd, "GPKGRAM")
        K = run_gram(be, "f64", be.upload(X), 1, ls=one, sf2=1.0, diag=0.0)
        assert N <= 2816 and assert_form(capfd, "f64", N, 1)[1] == 1
        got = K.cpu().numpy()[:N, :N]
    else:
        got = run_cross(be, "f64", X, X, one, 1.0, 0).cpu().numpy()[:N, :N]
    k = np.abs(idx[:, None] - idx[None, :])
    c = cls[k]
    assert (c == 0).sum() > 4e6 and (c == 1).sum() > 1e4 and (c == 2).sum() > 500
    normal = c == 0
    rel = np.abs((got[normal] - hi[k][normal]) - lo[k][normal]) / hi[k][normal]
    sub = c == 1
    units = np.abs(np.ldexp(got[sub], 1074) - (np.ldexp(hi[k][sub], 1074) + lo[k][sub]))
    print(f"exp fp64 through {entry}: normal range worst {rel.max() * 2.0 ** 52:.3f} x 2^-52 relative (at i = {k[normal][rel.argmax()]}), "
          f"subnormal range worst {units.max():.2f} units of 2^-1074, {int((c == 2).sum())} entries under the clamp")
    assert rel.max() <= 2.0 ** -52
    assert units.max() <= 2.0
    assert not got[c == 2].any()
    dup = (k == 0) & ~np.eye(N, dtype=bool)
    assert dup.sum() == 80 and np.all(got[dup] == 1.0) and np.all(np.diag(got) == 1.0)


# ---- H. the split cross panel ---------------------------------------------------------------------------------------------
SPLIT_CASES = [(300, 70, d) for d in range(1, 17)] + [(129, 257, 9), (1000, 1, 9)]


@pytest.mark.parametrize("sf2", [1.3, 0.004])
@pytest.mark.parametrize("N,M,D", SPLIT_CASES)
def test_split_cross_panel(be, N, M, D, sf2):
    """cross_split2_kernel<D> through gpk_predict_var_inv_split2 with W = I (split by gpk_split2_rows): the panel it leaves in
    `work2`, decoded, must be the two fp16 parts of gpk_cross_gram_t's fp32 entries times k_scale ("same arithmetic per entry as
    cross_t_kernel"), and the variance is kss - sum_j k(xq, x_j)^2."""
    import torch
    rng = np.random.default_rng(1000 * N + 16 * M + D)
    X, Xq = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    ls = ls_of(D)
    Np, Mp = padded(N), padded(M)
    k_scale = 2.0 ** (14 - int(np.floor(np.log2(sf2))))
    assert k_scale == {1.3: 2.0 ** 14, 0.004: 2.0 ** 22}[sf2]
    Xd, Xqd = be.upload(X, torch.float32), be.upload(Xq, torch.float32)
    eye = torch.eye(Np, dtype=torch.float32, device=be.device)
    W2 = torch.zeros((Np * Np * 4,), dtype=torch.uint8, device=be.device)
    scales = be.empty((Np // 128,), torch.float32)
    work2 = be.empty((Np * Mp * 4,), torch.uint8)
    var = be.empty((M,), torch.float64)
    ref = O.rbf_cross(Xq.astype(np.float32).astype(np.float64), X.astype(np.float32).astype(np.float64), ls, sf2)     # (M, N)
    ssq = np.einsum("ij,ij->i", ref, ref)
    kss = 2.0 * float(ssq.max())
    be.bind_stream()
    be.check(be.lib.gpk_split2_rows(be.h, _p(eye), Np, Np, _p(scales), _p(W2)))
    be.check(be.lib.gpk_predict_var_inv_split2(be.h, _p(Xd), N, D, _dp(ls), sf2, _p(W2), _p(scales), Np, _p(Xqd), M, kss, 0.0,
                                               _p(work2), _p(var)))
    be.sync()
    assert bool((scales == 32768.0).all())
    h0, h1 = decode_split2_panel(work2.cpu().numpy(), Mp, Np)
    x = run_cross(be, "f32", Xq, X, ls, sf2, 0).cpu().numpy() * np.float32(k_scale)          # exact: a power of two
    assert x.dtype == np.float32 and np.all(np.isfinite(x)) and x.max() < 32768.0
    e = np.max(np.abs(x[:M, :N].astype(np.float64) / k_scale - ref)) / sf2
    w0 = x.astype(np.float16)
    w1 = (x - w0.astype(np.float32)).astype(np.float16)
    n0, n1 = int((h0 != w0.astype(np.float64)).sum()), int((h1 != w1.astype(np.float64)).sum())
    back = np.max(np.abs(h0 + h1 - x.astype(np.float64)) / np.maximum(2.0 ** -23 * np.abs(x), 2.0 ** -25))
    print(f"split panel N {N} M {M} D {D} sf2 {sf2}: entries {e:.2e} of sf2, h0 differs in {n0}, h1 in {n1} of {h0.size}, "
          f"|h0 + h1 - x| at most {back:.2f} of max(2^-23 |x|, 2^-25)")
    assert e <= F32_BAR
    assert n0 == 0 and n1 == 0, "the panel must hold fp16(x) and fp16(x - h0) of the cross kernel's own entries"
    assert not h0[M:].any() and not h1[M:].any() and not h0[:, N:].any() and not h1[:, N:].any()
    v = var.cpu().numpy()
    want = kss - ssq
    es = np.max(np.abs(np.sqrt(v) - np.sqrt(want)) / np.sqrt(want))
    print(f"split panel N {N} M {M} D {D} sf2 {sf2}: std of the variance launch on W = I {es:.2e}")
    assert es < 1e-3                                                            # the bar of test_variance_16bit_split_paths


# ---- I. K4 instantiations: gpk_predict_mean -----------------------------------------------------------------------------
_mean_ref = {}


def mean_case(N, M, D, P):
    """(X, alpha, Xq, ls, y_mean, y_std, the oracle's mean), evaluated once per shape."""
    if (N, M, D, P) not in _mean_ref:
        rng = np.random.default_rng(31 * N + 7 * M + 16 * D + P)
        X, Xq, alpha = rng.standard_normal((N, D)), rng.standard_normal((M, D)), rng.standard_normal((N, P))
        ym, ys = rng.standard_normal(P), 0.5 + rng.random(P)
        ls = ls_of(D)
        st = O.FitState(X, None, alpha, ym, ys, ls, SF2, 0.0, 0.0)
        _mean_ref[(N, M, D, P)] = (X, alpha, Xq, ls, ym, ys, O.predict(st, Xq))
    return _mean_ref[(N, M, D, P)]


def run_mean(be, capfd, dtype, N, M, D, P):
    X, alpha, Xq, ls, ym, ys, want = mean_case(N, M, D, P)
    t = _tdt(dtype)
    Xd, ad, qd = be.upload(X, t), be.upload(alpha, t), be.upload(Xq, t)
    out = be.empty((M, P), t)
    log_lines(capfd, "GPKMEAN")
    be.bind_stream()
    be.check(be.lib.gpk_predict_mean(be.h, _code(dtype), _p(Xd), _p(ad), N, D, P, _dp(ls), SF2, _dp(ym), _dp(ys), _p(qd), M, _p(out)))
    be.sync()
    gran, S, chunk = mean_form(dtype, N, M)
    lines = log_lines(capfd, "GPKMEAN")
    assert lines == [[dtype, str(N), str(M), str(D), f"P{P}", f"d{(D + 3) // 4}", f"p{(P + 3) // 4}", f"gran{gran}", f"s{S}", f"chunk{chunk}"]], lines
    got = out.double().cpu().numpy()
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want))), (gran, S, chunk)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("M", [3, 600])
@pytest.mark.parametrize("D", [1, 4, 5, 8, 9, 12, 13, 16])
def test_predict_mean_instantiations(be, capfd, dtype, M, D):
    """Every (d4, p4) of predict_mean_kernel at both edges of each: fp64 within 1e-11 of the oracle (test_predict_mean_fp64_fp32),
    fp32 within 1e-4 of the largest mean (test_predict_mean_mfma)."""
    worst = 0.0
    for P in (1, 4, 5, 8, 9, 12, 13, 16):
        e, form = run_mean(be, capfd, dtype, 333, M, D, P)
        assert form[0] == (32 if M == 3 else 128)
        assert e < (1e-11 if dtype == "f64" else 1e-4), (P, e)
        worst = max(worst, e)
    print(f"predict_mean {dtype} N 333 M {M} D {D}, P in 1 .. 16: worst {worst:.2e} of the largest mean, form {form}")


@pytest.mark.parametrize("M", [3, 600])
def test_predict_mean_fp32_large_n(be, capfd, M):
    """fp32 at N = 5000: 157 chunks of 32 rows (M = 3) and 40 of 128 (M = 600), the last one ragged (8 rows), two-level sums.
    (Neither reaches the 2048-row cap: so few queries already split the training set further - see the next test.)"""
    e, form = run_mean(be, capfd, "f32", 5000, M, 9, 3)
    assert form == ((128, 40, 128) if M == 600 else (32, 157, 32)) and 5000 % 128 == 8
    print(f"predict_mean f32 N 5000 M {M}: form {form}: {e:.2e} of the largest mean")
    assert e < 1e-4


def test_predict_mean_fp32_chunk_cap(be, capfd):
    """The fp32 2048-row cap binds once the query blocks alone fill the grid: M = 600 000 queries (1172 blocks) would take the
    5000 rows in two chunks, the cap makes it three of 1792 (14 rounds of 128; the last chunk 1416 rows: 11 rounds and a ragged
    one of 8).  The reference is evaluated on the device in panels (`rbf_panel` on the fp32-rounded inputs)."""
    import torch
    N, M, D, P = 5000, 600000, 9, 3
    assert mean_form("f32", N, M) == (128, 3, 1792) and mean_form("f64", N, M) == (128, 2, 2560)
    rng = np.random.default_rng(5)
    X, Xq, alpha = rng.standard_normal((N, D)), rng.standard_normal((M, D)), rng.standard_normal((N, P))
    ym, ys, ls = rng.standard_normal(P), 0.5 + rng.random(P), ls_of(D)
    Xd, ad, qd = be.upload(X, torch.float32), be.upload(alpha, torch.float32), be.upload(Xq, torch.float32)
    out = be.empty((M, P), torch.float32)
    log_lines(capfd, "GPKMEAN")
    be.bind_stream()
    be.check(be.lib.gpk_predict_mean(be.h, _code("f32"), _p(Xd), _p(ad), N, D, P, _dp(ls), SF2, _dp(ym), _dp(ys), _p(qd), M, _p(out)))
    be.sync()
    assert log_lines(capfd, "GPKMEAN") == [["f32", str(N), str(M), str(D), "P3", "d3", "p1", "gran128", "s3", "chunk1792"]]
    ymd, ysd = be.upload(ym), be.upload(ys)
    worst, largest = 0.0, 0.0
    for r0 in range(0, M, 8192):
        want = rbf_panel(qd[r0:r0 + 8192].double(), Xd.double(), ls, SF2) @ ad.double() * ysd + ymd
        worst = max(worst, float((out[r0:r0 + 8192].double() - want).abs().max()))
        largest = max(largest, float(want.abs().max()))
    print(f"predict_mean f32 N {N} M {M}: three chunks of 1792 rows: {worst / largest:.2e} of the largest mean")
    assert worst < 1e-4 * largest


# ---- J. K4 instantiations: gpk_predict_mean_multi -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("M", [3, 600])
@pytest.mark.parametrize("D", [1, 4, 5, 16])
def test_predict_mean_multi_instantiations(be, capfd, dtype, M, D):
    """Column b of the fused launch against gpk_predict_mean of model b alone, per-model length-scales and sf2.  fp64: 1e-12 of
    the largest mean, the bar tests/test_gpu_axis_jac.py holds the fused per-axis mean to against the per-model calls (the
    fused kernel weights the squared raw differences by 1 / ls^2 instead of differencing divided coordinates: a few ulps of
    d^2 per term, 333 terms); fp32: each side within 1e-4 of the largest mean of the fp64 oracle, so 2e-4 between them."""
    N = 333
    t = _tdt(dtype)
    worst = 0.0
    for B in (1, 4, 5, 8):
        rng = np.random.default_rng(1000 * D + 10 * B + M)
        X, Xq, alpha = rng.standard_normal((N, D)), rng.standard_normal((M, D)), rng.standard_normal((N, B))
        ls = ls_of(D)[None, :] * (1.0 + 0.3 * rng.random((B, D)))
        sf2, ym, ys = 0.5 + rng.random(B), rng.standard_normal(B), 0.5 + rng.random(B)
        Xd, ad, qd = be.upload(X, t), be.upload(alpha, t), be.upload(Xq, t)
        out = be.empty((M, B), t)
        log_lines(capfd, "GPKMEAN")
        be.bind_stream()
        be.check(be.lib.gpk_predict_mean_multi(be.h, _code(dtype), _p(Xd), _p(ad), N, D, B, _dp(np.ascontiguousarray(ls)), _dp(sf2), _dp(ym),
                                               _dp(ys), _p(qd), M, _p(out)))
        be.sync()
        gran, S, chunk = mean_form(dtype, N, M, multi=True)
        assert log_lines(capfd, "GPKMEAN") == [[dtype, str(N), str(M), str(D), f"B{B}", f"d{(D + 3) // 4}", f"p{1 if B <= 4 else 2}",
                                                f"gran{gran}", f"s{S}", f"chunk{chunk}"]]
        got = out.double().cpu().numpy()
        for b in range(B):
            ab = be.upload(np.ascontiguousarray(alpha[:, b:b + 1]), t)
            one = be.empty((M, 1), t)
            be.check(be.lib.gpk_predict_mean(be.h, _code(dtype), _p(Xd), _p(ab), N, D, 1, _dp(np.ascontiguousarray(ls[b])), float(sf2[b]),
                                             _dp(ym[b:b + 1]), _dp(ys[b:b + 1]), _p(qd), M, _p(one)))
            be.sync()
            ref = one.double().cpu().numpy()[:, 0]
            e = float(np.max(np.abs(got[:, b] - ref)) / np.max(np.abs(ref)))
            assert e < (1e-12 if dtype == "f64" else 2e-4), (B, b, e)
            worst = max(worst, e)
        log_lines(capfd, "GPKMEAN")
    print(f"predict_mean_multi {dtype} N {N} M {M} D {D}, B in 1 .. 8: worst {worst:.2e} of the largest mean against the per-model launch")


# ---- K. gpk_colsumsq ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("Np,Mp,ldb", [(128, 128, 128), (130, 128, 256), (897, 256, 256), (1000, 384, 512), (4099, 128, 128)])
def test_colsumsq_exact(be, dtype, Np, Mp, ldb):
    """Integer entries in [-3, 3]: the sums are exact in any order.  Odd rows per slab (65, 67), both thread halves' tails, a
    pitch whose columns hold NaN (a read of one would show), the bytes after the result untouched."""
    import torch
    S, rows_per = colsumsq_form(Np, Mp)
    assert rows_per % 2 == (Np != 128)
    B = np.full((Np, ldb), np.nan)
    B[:, :Mp] = np.random.default_rng(Np + Mp).integers(-3, 4, size=(Np, Mp))
    Bd = be.upload(B, _tdt(dtype))
    out = torch.full((Mp + 64,), float("nan"), dtype=torch.float64, device=be.device)
    be.bind_stream()
    be.check(be.lib.gpk_colsumsq(be.h, _code(dtype), _p(Bd), Np, Mp, ldb, _p(out)))
    be.sync()
    got = out.cpu().numpy()
    assert np.array_equal(got[:Mp], (B[:, :Mp] ** 2).sum(axis=0)) and np.isnan(got[Mp:]).all()
