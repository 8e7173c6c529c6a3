"""Every launch form of the 16-bit variance kernels (gpk_k5split.hip) called directly through the C ABI on operands the test builds
itself - no fitted model - against the fp64 reference, the launch-rule mirrors and the bars of tests/test_k5_refs.py:

A  fp16 x 2, gpk_predict_var_inv_split2 on gpk_split2_rows' operand: k5_direct_kernel<1>, <2> (by the rule and by option
   k5_split2_tile = 3) and <4> (by the rule and forced), padded and unpadded walks, groups that straddle bands, the ragged last
   band, one tile column, a single data row, D = 16; the three tile heights on one operand;
B  the fp64-source splitters gpk_split2_rows_f64 / gpk_split2_rows_f64_absmax: NaN above the diagonal of the source, a destination
   that starts as NaN, the scales and the written chunks of gpk_split2_rows bit for bit, the launch on that operand for every tile
   height (it never reads what the splitter leaves unwritten), and the block scales at their edges (zeros, rounded to zero, clamped);
C  bf16 x 3, gpk_predict_var_inv_split on gpk_split3's operand: k5_split_kernel<4> and <2>, groups that run to the group's longest
   k-range over one and two bands and groups whose tiles keep their own (more than two bands), the ragged last band;
D  the packed serving step gpk_predict_mean_var_split2;      E  the refusals.

The operand is a DENSE lower-triangular W with rows of unit length (test_k5_refs.case_operands): every 32-row block and every k16
step of it carries its share of S_m = sum_r (sum_k W_rk K*_mk)^2, so a tile whose k-range stops a step short, a wave on a
neighbour's row block or a dropped cross product moves S by more than the bar.  What is compared is S itself, e = max_m
|S_gpu - S| / S with S_gpu = kss - var (kss = 2 max S, floor 0: nothing clipped), against bar = min(128 / Np^2, e_cross / 4) from the
reference side alone (test_k5_refs.case_bar).  A fresh handle with option `k5_log`; every case computes its form from the mirrors,
asserts the features it claims and the library's own GPKK5 line, runs twice and asserts identical bits; outputs start as NaN.

Predicted from reading the code, and found:
* predicted: nothing wrong in the index arithmetic of either walk (the mirrors visit every tile once for every case, CPU side), the
  poisoned chunks right of the diagonal tile never read, the bf16 x 3 lockstep ranges inside W's zero band.  Found: so it is - every
  case passed at the first run and the kernels are unchanged;
* a block of W "scaled by 2^-110" is NOT rounded to zero in fp32 (entries near 2^-115 are normal numbers): its scale clamps at 2^100
  like the 2^-90 block's.  The block-scale case keeps both and adds a block scaled by 2^-160 that does round to zero (scale 1);
* with a single data row (case h) every live entry of W is +-1 and a1 = 0: the a1 b0 product cannot be told from its absence, and
  the case's bar comes from the other first-order product (test_k5_refs.case_bar).

Measured on an MI355X, worst case per group (e / the complete emulation's error / bar; every case prints its own):
* A, fp16 x 2: e between 9.5e-8 (h) and 2.2e-7 (e: 2.2e-7 / 7.9e-8 / 2.9e-6); closest to its bar c: 1.9e-7 / 5.3e-8 / 9.7e-7.  The
  launch stands 1.4 to 3.6 times above the emulation: K* is computed in fp32 on the device (gpk_cross_split2, up to 1.9e-7 sf2 per
  entry, tests/test_gpu_gram_forms.py) where the emulation rounds the fp64 value once.  Case e on 128- and 256-row tiles: 1.8e-7 and
  1.9e-7, 1.3e-7 and 1.2e-7 from the 512-row launch;
* B: scales, written chunks and variances identical bit for bit in all six runs (b, d, g x two entries), 557 056 / 61 440 / 491 520
  chunks left as NaN; the block-scale case 3.4e-7 / 2.6e-7 / 8.5e-6, scales 2^15, 1, 2^100, 2^100, 2^-23, 1;
* C, bf16 x 3: e between 1.6e-7 and 2.0e-7 (N 2400 M 350: 2.0e-7 / 1.6e-8 / 6.8e-6) - again K*'s fp32 arithmetic (gpk_cross_gram_t,
  2.6e-7 sf2 per entry), ten times the product's own error, the same whichever k-range rule a group follows;
* D: bit for bit; 150 of 300 rows below the median as recheck_below, 300 of 300 at the floor.
The same cases run against five deliberately wrong builds of gpk_k5split.hip (fp16 x 2 without a1 b0: e 4.9e-6 .. 1.6e-5; wave 3 one
k16 step short: 3.7e-4 .. 6.7e-3; wave 3 on wave 2's row block: 1.7e-2 .. 9.7e-2; bf16 x 3 without a1 b0: 2.5e-5 .. 6.9e-5; its
k-range 128 columns short: 5.9e-3 .. 8.7e-2): each failed every group A (but h, whose only live column is k = 0 with a1 = 0) or
group C case, the block-scale case, and the third the 512-row launch on the fp64-source operand.
"""
import ctypes as C
import sys

import numpy as np
import pytest

from test_gram_refs import padded
from test_k5_refs import (DIRECT_CASES, DIRECT_CLAIMS, SCALE_CASE, SCALE_WANT, SF2, SPLIT_CASES, SPLIT_D, case_bar, case_operands,
                          decode_split2_rows, k5_direct_form, k5_split_form, kstar, ls_of, rel_err, s_reference, scale_case_factor, split2_parts,
                          split2_scales, split_walk)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from unmanned_aerial_vehicles_amd.device import Backend
    b = Backend(0).set_options(k5_log=1)
    yield b
    b.lib.gpk_destroy(b.h)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _dp(a):
    from unmanned_aerial_vehicles_amd import _lib
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_lib._dp)


def k5_lines(capfd):
    """The words of the GPKK5 lines (option k5_log) written to stderr since the last call."""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    return [ln.split()[1:] for ln in cap.err.splitlines() if ln.startswith("GPKK5 ")]


def nan_bytes(be, n):
    """n bytes of 0xFF on the device: NaN as fp16, bf16, fp32 and fp64 alike."""
    import torch
    return torch.full((n,), 255, dtype=torch.uint8, device=be.device)


def nan_f64(be, n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device=be.device)


_dev = {}


def dev_case(be, N, M, D, W32=None, key=None):
    """The operands of a case on the device and its reference, evaluated once: X, Xq, W (fp32), S (fp64, NumPy), kss = 2 max S."""
    import torch
    k = (N, M, D, key)
    if k not in _dev:
        X, Xq, ls, W = case_operands(N, M, D)
        W = W if W32 is None else W32
        Np = W.shape[0]
        Wd = be.upload(W.copy(), torch.float32)                    # (the cached factor is read-only: torch wants a writable array)
        S = s_reference(Wd, kstar(X, Xq, ls, Np, device=be.device))
        assert np.all(np.isfinite(S)) and S.min() > 0.0
        _dev[k] = dict(N=N, M=M, D=D, Np=Np, Mp=padded(M), ls=ls, X=be.upload(X, torch.float32), Xq=be.upload(Xq, torch.float32), W=Wd,
                       S=S, kss=2.0 * float(S.max()))
    return _dev[k]


def split2_operand(be, c):
    """(W2, scales) of gpk_split2_rows on the case's W, once per case."""
    import torch
    if "W2" not in c:
        Np = c["Np"]
        W2, scales = nan_bytes(be, Np * Np * 4), be.empty((Np // 128,), torch.float32).fill_(float("nan"))
        be.bind_stream()
        be.check(be.lib.gpk_split2_rows(be.h, _p(c["W"]), Np, Np, _p(scales), _p(W2)))
        be.sync()
        c["W2"], c["scales"] = W2, scales
    return c["W2"], c["scales"]


def run_direct(be, capfd, c, opt, W2, scales, kss=None, floor=0.0):
    """gpk_predict_var_inv_split2 under option k5_split2_tile = opt, twice, into NaN buffers; the GPKK5 line of each launch asserted
    against the mirror.  Returns (var[:M] as NumPy, the form)."""
    import torch
    N, M, D, Np, Mp = c["N"], c["M"], c["D"], c["Np"], c["Mp"]
    form = k5_direct_form(Np, Mp, opt)
    ab, bh, per, per_pad, ntmT, nst, grid = form
    want = ["direct", f"rows{128 * ab}", f"ntmT{ntmT}", f"ntn{Mp // 128}", f"nst{nst}", f"pad{per_pad}", f"grid{grid}"]
    out = []
    be.check(be.lib.gpk_set_option(be.h, b"k5_split2_tile", opt))
    try:
        for _ in range(2):
            work2, var = nan_bytes(be, Np * Mp * 4), nan_f64(be, Mp + 64)
            k5_lines(capfd)
            be.bind_stream()
            be.check(be.lib.gpk_predict_var_inv_split2(be.h, _p(c["X"]), N, D, _dp(c["ls"]), SF2, _p(W2), _p(scales), Np, _p(c["Xq"]), M,
                                                       c["kss"] if kss is None else kss, floor, _p(work2), _p(var)))
            be.sync()
            lines = k5_lines(capfd)
            assert lines == [want], (lines, want)
            assert bool(torch.isnan(var[M:]).all()), "nothing behind row M may be written"
            out.append(var[:M].cpu().numpy())
    finally:
        be.check(be.lib.gpk_set_option(be.h, b"k5_split2_tile", 0))
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64)), "two runs must give identical bits"
    return out[0], form


def s_err(c, var):
    assert np.all(np.isfinite(var)) and var.min() > 0.0, "kss = 2 max S: nothing may be clipped or NaN"
    return rel_err(c["kss"] - var, c["S"])


# ---- A. fp16 x 2 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DIRECT_CASES))
def test_direct_forms(be, capfd, name):
    N, M, D, opt = DIRECT_CASES[name]
    c = dev_case(be, N, M, D)
    W2, scales = split2_operand(be, c)
    var, (ab, bh, per, per_pad, ntmT, nst, grid) = run_direct(be, capfd, c, opt, W2, scales)
    cl = DIRECT_CLAIMS[name]
    assert (ab, ntmT, per, per_pad, ntmT // bh, ntmT % bh) == (cl["ab"], cl["ntmT"], cl["per"], cl["per_pad"], cl["nfull"], cl["hlast"])
    W = case_operands(N, M, D)[3]
    want_sc = split2_scales(W)
    assert np.array_equal(scales.cpu().numpy(), want_sc)
    if c["Np"] <= 1280:          # gpk_split2_rows' operand, decoded: fp16(x s) and fp16(x s - h0) of every entry, zeros above the diagonal
        h0, h1 = decode_split2_rows(W2.cpu().numpy(), c["Np"])
        w0, w1 = split2_parts(W * np.repeat(want_sc, 128)[:, None])
        assert np.array_equal(h0, w0.astype(np.float64)) and np.array_equal(h1, w1.astype(np.float64))
    bar, e_full, e_cross, which = case_bar("direct", N, M, D)
    e = s_err(c, var)
    print(f"direct {name}: N {N} M {M} D {D} option {opt}: rows {128 * ab} ntmT {ntmT} per {per} -> {per_pad} nst {nst} grid {grid}: "
          f"e {e:.2e}, emulation {e_full:.2e}, without {which} {e_cross:.2e}, bar {bar:.2e}")
    assert e <= bar
    c["var", opt] = var


def test_direct_tile_heights_agree(be, capfd):
    """Case e's operands (512-row tiles by the rule) on 128-row tiles (option 1) and 256-row tiles (option 3): each within the
    case's bar of the reference and of option 0."""
    N, M, D, _ = DIRECT_CASES["e"]
    c = dev_case(be, N, M, D)
    W2, scales = split2_operand(be, c)
    bar = case_bar("direct", N, M, D)[0]
    v = {}
    for opt, ab in ((0, 4), (1, 1), (3, 2), (4, 4)):          # (a value outside 0 .. 3 is taken as 0)
        v[opt], form = run_direct(be, capfd, c, opt, W2, scales)
        assert form[0] == ab
    assert np.array_equal(v[4].view(np.uint64), v[0].view(np.uint64))
    for opt in (1, 3):
        e, d = s_err(c, v[opt]), rel_err(c["kss"] - v[opt], c["kss"] - v[0])
        print(f"direct e, option {opt}: e {e:.2e}, against option 0 {d:.2e}, bar {bar:.2e}")
        assert e <= bar and d <= bar


# ---- B. the fp64-source splitters ---------------------------------------------------------------------------------------
def written_chunks(Np):
    """Which 16-byte chunks of a fragment-order operand split2_f64_kernel writes: those of (32-row block rb, k16 block kb) up to the
    row's diagonal 128-tile."""
    KB = Np // 16
    pair = np.arange(Np // 32 * KB)                       # (rb, kb) -> 128 chunks each (two parts of 64)
    rb, kb = pair // KB, pair % KB
    return np.repeat(kb * 16 < ((rb * 32) // 128 + 1) * 128, 128)


def f64_source(be, W32):
    """The fp32 factor as fp64 on the device with NaN everywhere strictly above the diagonal."""
    import torch
    W64 = W32.astype(np.float64)
    W64[np.triu_indices(W64.shape[0], 1)] = np.nan
    return be.upload(W64, torch.float64)


def split_f64(be, W64d, Np, absmax=None):
    import torch
    dst = nan_bytes(be, Np * Np * 4)
    be.bind_stream()
    if absmax is None:
        scales = be.empty((Np // 128,), torch.float32).fill_(float("nan"))
        be.check(be.lib.gpk_split2_rows_f64(be.h, _p(W64d), Np, Np, _p(scales), _p(dst)))
    else:
        scales = be.upload(absmax, torch.float32)
        be.check(be.lib.gpk_split2_rows_f64_absmax(be.h, _p(W64d), Np, Np, _p(scales), _p(dst)))
    be.sync()
    return dst, scales


@pytest.mark.parametrize("name", ["b", "d", "g"])
def test_split2_f64_sources(be, capfd, name):
    N, M, D, opt = DIRECT_CASES[name]
    c = dev_case(be, N, M, D)
    Np = c["Np"]
    W2, scales = split2_operand(be, c)
    W32 = case_operands(N, M, D)[3]
    W64d = f64_source(be, W32)
    absmax = np.abs(np.tril(W32)).reshape(Np // 128, -1).max(axis=1).astype(np.float32)
    ref_var = c["var", opt] if ("var", opt) in c else run_direct(be, capfd, c, opt, W2, scales)[0]
    want = W2.cpu().numpy().reshape(-1, 16)
    wr = written_chunks(Np)
    assert wr.size == want.shape[0] and 0 < int((~wr).sum()) == sum(128 * (Np // 16 - 8 * (rb // 4 + 1)) for rb in range(Np // 32))
    for how, am in (("f64", None), ("f64_absmax", absmax)):
        dst, sc = split_f64(be, W64d, Np, am)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), scales.cpu().numpy().view(np.uint32)), how
        got = dst.cpu().numpy().reshape(-1, 16)
        assert np.array_equal(got[wr], want[wr]), f"{how}: the written chunks must be gpk_split2_rows' bit for bit"
        assert bool((got[~wr] == 255).all()), f"{how}: the chunks right of the diagonal tile are documented as left unwritten"
        var, form = run_direct(be, capfd, c, opt, dst, sc)
        assert form[0] == DIRECT_CLAIMS[name]["ab"]
        assert np.array_equal(var.view(np.uint64), ref_var.view(np.uint64)), f"{how}: the launch must never read an unwritten chunk"
        print(f"split2_rows_{how} on case {name} (rows {128 * form[0]}): {int(wr.sum())} chunks identical, {int((~wr).sum())} left as NaN, same variance bits")


def test_split2_block_scales(be, capfd):
    """Blocks of zeros, of entries that round to zero in fp32 (x 2^-160), of entries whose scale would exceed 2^100 (x 2^-110,
    x 2^-90: clamped) and of large entries (x 2^40), from the fp32 and the fp64 source: the scales of the mirror bit for bit, a finite
    result within the bar of the reference on the fp32-rounded W."""
    N, M, D = SCALE_CASE
    W64, W32 = scale_case_factor()
    c = dev_case(be, N, M, D, W32=W32, key="scales")
    Np = c["Np"]
    bar, e_full, e_cross, _ = case_bar("direct", N, M, D, 0, True)
    want_sc = split2_scales(W32)
    assert [float(want_sc[b]) for b in (1, 2, 3, 5)] == [SCALE_WANT[b] for b in (1, 2, 3, 5)]
    W2, scales = split2_operand(be, c)
    src = W64.copy()
    src[np.triu_indices(Np, 1)] = np.nan
    import torch
    dst, sc64 = split_f64(be, be.upload(src, torch.float64), Np)
    for how, s in (("fp32", scales), ("fp64", sc64)):
        assert np.array_equal(s.cpu().numpy().view(np.uint32), want_sc.view(np.uint32)), (how, s)
    v32, _ = run_direct(be, capfd, c, 0, W2, scales)
    v64, _ = run_direct(be, capfd, c, 0, dst, sc64)
    e = s_err(c, v32)
    print(f"block scales {want_sc}: e {e:.2e}, emulation {e_full:.2e}, bar {bar:.2e}")
    assert e <= bar and np.array_equal(v32.view(np.uint64), v64.view(np.uint64))


# ---- C. bf16 x 3 ------------------------------------------------------------------------------------------------------
def split3_operand(be, c):
    if "W3" not in c:
        Np = c["Np"]
        W3 = nan_bytes(be, Np * Np * 6)
        be.bind_stream()
        be.check(be.lib.gpk_split3(be.h, _p(c["W"]), Np, Np, Np, _p(W3)))
        be.sync()
        c["W3"] = W3
    return c["W3"]


_w3 = {}


@pytest.mark.parametrize("N,M", list(SPLIT_CASES))
def test_split_forms(be, capfd, N, M):
    import torch
    c = dev_case(be, N, M, SPLIT_D)
    Np, Mp = c["Np"], c["Mp"]
    if N not in _w3:                                 # (one split operand per factor, shared by its cases)
        _w3[N] = split3_operand(be, c)
    W3 = _w3[N]
    wr, gsz, bh, ntmT, nst, grid = k5_split_form(Np, Mp)
    want_wr, want_lock, want_own = SPLIT_CASES[(N, M)]
    live = [w for w in split_walk(Np, Mp) if w is not None]
    assert wr == want_wr and sorted({w[2] for w in live if w[4]}) == want_lock and sorted({w[2] for w in live if not w[4]}) == want_own
    assert ntmT % bh == {2304: 1, 2432: 3}[Np]                              # the ragged last band: one tile row of 256, three of 128
    want = ["split", f"rows{64 * wr}", f"ntmT{ntmT}", f"ntn{Mp // 128}", f"nst{nst}", "pad0", f"grid{grid}"]
    out = []
    for _ in range(2):
        work = torch.full((Mp * Np,), float("nan"), dtype=torch.float32, device=be.device)
        work3, var = nan_bytes(be, Mp * Np * 6), nan_f64(be, Mp + 64)
        k5_lines(capfd)
        be.bind_stream()
        be.check(be.lib.gpk_predict_var_inv_split(be.h, _p(c["X"]), N, SPLIT_D, _dp(c["ls"]), SF2, _p(W3), Np, _p(c["Xq"]), M, c["kss"], 0.0,
                                                  _p(work), _p(work3), _p(var)))
        be.sync()
        lines = k5_lines(capfd)
        assert lines == [want], (lines, want)
        assert bool(torch.isnan(var[M:]).all())
        out.append(var[:M].cpu().numpy())
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64)), "two runs must give identical bits"
    bar, e_full, e_cross, _ = case_bar("split", N, M, SPLIT_D)
    e = s_err(c, out[0])
    print(f"split N {N} M {M}: rows {64 * wr} ntmT {ntmT} nst {nst} grid {grid}, lockstep {want_lock}, own {want_own}: "
          f"e {e:.2e}, emulation {e_full:.2e}, without a1b0 {e_cross:.2e}, bar {bar:.2e}")
    assert e <= bar


# ---- D. the packed step -----------------------------------------------------------------------------------------------
def test_packed_step(be, capfd):
    import torch
    N, M, D, opt = DIRECT_CASES["b"]
    P, GUARD = 3, 64
    c = dev_case(be, N, M, D)
    Np, Mp = c["Np"], c["Mp"]
    W2, scales = split2_operand(be, c)
    var = c["var", opt] if ("var", opt) in c else run_direct(be, capfd, c, opt, W2, scales)[0]
    rng = np.random.default_rng(4)
    alpha = be.upload(rng.standard_normal((N, P)), torch.float32)
    ym, ys, center = rng.standard_normal(P), 0.5 + rng.random(P), np.zeros(D)
    mean = torch.full((M * P,), float("nan"), dtype=torch.float32, device=be.device)
    be.bind_stream()
    be.check(be.lib.gpk_predict_mean_mfma(be.h, _p(c["X"]), _p(alpha), N, D, P, _dp(c["ls"]), SF2, _dp(center), _dp(ym), _dp(ys), _p(c["Xq"]), M, _p(mean)))
    be.sync()
    mean = mean.cpu().numpy().reshape(M, P)
    assert np.all(np.isfinite(mean))
    form = k5_direct_form(Np, Mp, 0)
    want_line = ["direct", f"rows{128 * form[0]}", f"ntmT{form[4]}", f"ntn{Mp // 128}", f"nst{form[5]}", f"pad{form[3]}", f"grid{form[6]}"]
    recheck = float(np.median(var))
    floor = 0.125
    assert floor < recheck
    for kss, fl in ((c["kss"], 0.0), (0.5 * float(c["S"].min()), floor)):
        out = nan_f64(be, M * 2 * P + GUARD)
        tmp = torch.full((M * P,), float("nan"), dtype=torch.float32, device=be.device)
        work2 = nan_bytes(be, Np * Mp * 4)
        low = torch.zeros((1,), dtype=torch.int32, device=be.device)
        k5_lines(capfd)
        be.bind_stream()
        be.check(be.lib.gpk_predict_mean_var_split2(be.h, _p(c["X"]), _p(alpha), N, D, P, _dp(c["ls"]), SF2, _dp(center), _dp(ym), _dp(ys), _p(W2),
                                                    _p(scales), Np, _p(c["Xq"]), M, kss, fl, _p(work2), _p(tmp), recheck, _p(low), _p(out)))
        be.sync()
        assert k5_lines(capfd) == [want_line]
        got = out.cpu().numpy()
        assert np.isnan(got[M * 2 * P:]).all(), "the guard band behind row M must stay untouched"
        got = got[:M * 2 * P].reshape(M, 2 * P)
        assert np.array_equal(got[:, :P], mean.astype(np.float64)), "the means must be gpk_predict_mean_mfma's"
        v = var if fl == 0.0 else np.full(M, floor)
        assert np.array_equal(got[:, P:], (v[:, None] * ys[None, :]) * ys[None, :]), "var * y_std^2 of the plain entry, bit for bit"
        count = int(low.item())       # (v is what the call returned: the assertion above holds bit for bit, and y_std^2 is applied after the gate)
        assert count == int((v < recheck).sum()) and (count == M if fl else 0 < count < M)
        print(f"packed step, kss {kss:.3g} floor {fl}: {count} of {M} rows below recheck_below")


# ---- E. refusals ------------------------------------------------------------------------------------------------------
def test_refusals(be, capfd):
    import torch
    from unmanned_aerial_vehicles_amd import _lib
    N, M, D = 300, 70, 6
    c = dev_case(be, N, M, D)
    Np, Mp = c["Np"], c["Mp"]
    W2, scales = split2_operand(be, c)
    W3 = split3_operand(be, c)
    work2, work3 = nan_bytes(be, Np * Mp * 4), nan_bytes(be, Np * Mp * 6)
    work = torch.full((Mp * Np,), float("nan"), dtype=torch.float32, device=be.device)
    var = nan_f64(be, Mp)
    X17 = torch.zeros((N, 17), dtype=torch.float32, device=be.device)
    alpha = torch.zeros((N, 2), dtype=torch.float32, device=be.device)
    tmp = torch.zeros((M * 2,), dtype=torch.float32, device=be.device)
    out = nan_f64(be, M * 4)
    one2 = np.ones(2)

    def direct(X=c["X"], N=N, D=D, ls=c["ls"], sf2=SF2, W2=W2, sc=scales, Np=Np, Xq=c["Xq"], M=M, work2=work2, var=var):
        return be.lib.gpk_predict_var_inv_split2(be.h, _p(X) if X is not None else None, N, D, _dp(ls), sf2, _p(W2) if W2 is not None else None,
                                                 _p(sc) if sc is not None else None, Np, _p(Xq) if Xq is not None else None, M, 1.0, 0.0,
                                                 _p(work2) if work2 is not None else None, _p(var) if var is not None else None)

    def split(X=c["X"], N=N, W3=W3, Np=Np, Xq=c["Xq"], M=M, work=work, work3=work3, var=var):
        q = lambda t: _p(t) if t is not None else None          # noqa: E731
        return be.lib.gpk_predict_var_inv_split(be.h, q(X), N, D, _dp(c["ls"]), SF2, q(W3), Np, q(Xq), M, 1.0, 0.0, q(work), q(work3), q(var))

    def packed(alpha=alpha, out=out, P=2, Np=Np):
        q = lambda t: _p(t) if t is not None else None          # noqa: E731
        return be.lib.gpk_predict_mean_var_split2(be.h, _p(c["X"]), q(alpha), N, D, P, _dp(c["ls"]), SF2, None, _dp(one2), _dp(one2), _p(W2), _p(scales),
                                                  Np, _p(c["Xq"]), M, 1.0, 0.0, _p(work2), _p(tmp), 0.0, None, q(out))

    calls = {
        "split2: Np != gpk_padded(N)": lambda: direct(Np=Np + 128), "split2: N = 0": lambda: direct(N=0), "split2: M = 0": lambda: direct(M=0),
        "split2: sf2 = 0": lambda: direct(sf2=0.0), "split2: sf2 < 0": lambda: direct(sf2=-1.3),
        "split2: D = 17": lambda: direct(X=X17, D=17, ls=ls_of(17)), "split2: D = 0": lambda: direct(D=0),
        "split2: null X": lambda: direct(X=None), "split2: null W2": lambda: direct(W2=None), "split2: null scales": lambda: direct(sc=None),
        "split2: null Xq": lambda: direct(Xq=None), "split2: null work2": lambda: direct(work2=None), "split2: null var": lambda: direct(var=None),
        "split: Np != gpk_padded(N)": lambda: split(Np=Np + 128), "split: null X": lambda: split(X=None), "split: null W3": lambda: split(W3=None),
        "split: null Xq": lambda: split(Xq=None), "split: null work": lambda: split(work=None), "split: null work3": lambda: split(work3=None),
        "split: null var": lambda: split(var=None),
        "packed: null alpha": lambda: packed(alpha=None), "packed: null out": lambda: packed(out=None), "packed: P = 0": lambda: packed(P=0),
        "packed: P = 17": lambda: packed(P=17), "packed: Np != gpk_padded(N)": lambda: packed(Np=Np + 128),
        "split2_rows: n % 128 != 0": lambda: be.lib.gpk_split2_rows(be.h, _p(c["W"]), Np - 64, Np, _p(scales), _p(W2)),
        "split2_rows: null W": lambda: be.lib.gpk_split2_rows(be.h, None, Np, Np, _p(scales), _p(W2)),
        "split2_rows_f64: n % 128 != 0": lambda: be.lib.gpk_split2_rows_f64(be.h, _p(out), 64, 64, _p(scales), _p(W2)),
        "split3: null dst": lambda: be.lib.gpk_split3(be.h, _p(c["W"]), Np, Np, Np, None),
    }
    k5_lines(capfd)
    be.bind_stream()

    def refused(what, call):
        rc = call()
        msg = be.lib.gpk_last_error(be.h).decode()
        assert rc == _lib.GPK_BAD_ARG and msg.startswith("bad argument") and len(msg) > len("bad argument: "), (what, rc, msg)

    for what, call in calls.items():
        refused(what, call)
    be.check(be.lib.gpk_batch_begin(be.h, 2))
    try:
        refused("split2: batched mode", direct)
        refused("split: batched mode", split)
        refused("packed: batched mode", packed)
    finally:
        be.check(be.lib.gpk_batch_end(be.h))
    be.sync()
    assert k5_lines(capfd) == [], "a refused call must not launch"
    assert bool(torch.isnan(var).all()) and bool(torch.isnan(out).all()) and bool((work2 == 255).all()) and bool((work3 == 255).all())
    # ... and the same arguments are accepted once nothing is wrong with them
    be.check(direct())
    be.check(split())
    be.sync()
    assert len(k5_lines(capfd)) == 2 and not bool(torch.isnan(var[:M]).any())
