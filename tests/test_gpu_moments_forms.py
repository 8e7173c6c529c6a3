"""Every launch form of the moment-matching kernels (K11, gpk_moments.hip: moments_setup_kernel, moments_row_mean_kernel,
moments_row_pair_kernel, moments_pair_kernel<P, SPLIT>, moments_finish_kernel, moments_keep_kernel, moments_grad_setup_kernel,
moments_grad_row_kernel, moments_pair_grad_kernel<PC, SPLIT>, moments_grad_finish_kernel) through the eight C entries
gpk_moments_host[_multi], gpk_moments_vjp_host[_multi], gpk_propagate_mm_host[_multi] and gpk_propagate_mm_grad_host[_multi], on
operands the test builds itself, against the extended-precision reference, the launch-rule mirror and the bars of
tests/test_moments_refs.py:

A  forward, one model: all 16 P at N = 65 with moments_query_groups = 1 (SPLIT false) and with the default; N in {1, 63, 64, 65, 128,
   255, 256, 257, 300} at P in {1, 5}; N = 1985 (G capped, sixteen workgroups with two tiles) and N = 3009 (two or three tiles) at P in
   {1, 3}; (nx, D) in {(1, 1), (1, 16), (16, 16), (2, 5), (3, 7) with P = 5}; R in {1, 2, 5, 32} with NQ in {1, 2, 3, R}; ldk = Np and
   Np + 2; the noise in and out; the clip; Sq NULL;
B  forward, batch: B = 1 .. 8 at N = 65; B = 8 at N = 257 (G U = 540); B = 2 at N = 1985; an input scaler with a negative scale; the
   clip on some models only;
C  adjoint: P in {1, 2, 8, 9, 16}; (D, nx) in {(1, 1), (5, 3), (16, 16), (16, 1)}; each seed NULL in turn; gcov not symmetric, gxcov
   with columns >= nx; the clip (the clipped queries keep their bits under another K^-1); N = 1985; batches;
D  the chains and their gradients: H in {1, 3}; x0, U, Sigma0 with 1 and with R rows; Sigma0 and Q NULL and not; coord a permutation
   with nx = B + 2; N in {65, 1985}; every stage checked from the chain's own traj[h], Sigma[h]; stage outputs with the bits of the
   query entry on the same rows;
E  six calls of different entries on one new handle, and the refusals of mm_models.

A fresh handle with the options `gram_log` (every call's GPKMM lines are asserted against `moments_form`, with the CU count the line
itself gives) and `debug_fill` (the scratch starts as NaN: a slot read before it is written shows).  X, alpha and K^-1 are views
into NaN-filled device buffers with 4 KiB of NaN before and behind; K^-1 is Np x ldk with NaN in its strict upper triangle, in rows
and columns >= N and in the pitch columns.  Every case runs twice and must give identical bits; its GPKMM lines equal the mirror's;
every output is within its bar of the reference; cov, dSq, Sigma and dSigma0 equal their transposes to the bit; the guards are
still NaN; e / bar is printed per output.

Predicted from reading the code, and found:
* predicted: the second tile of a workgroup (`t += G_`) accumulates into the slot it wrote (`first ? s : *dst + s`), the square-root
  recovery of (ti, tj) is exact up to t = 1175, and SPLIT = false is chosen from G U = 512 on - so N = 1985 and 3009 pass.  Found:
  so it is (e / bar at most 2.5e-4 there);
* predicted: every P from 1 to 16 and PC = 8 full, PC = 16 at P = 9 and 16 reduce their last chunk whatever NV mod 12 is (`v == NV -
  1`; NV = 11 at P = 4, 16 at P = 5, 137 at P = 16; the adjoint's NV = 12 at D = 5, nx = 3 and 153 at D = nx = 16).  Found: all pass;
* predicted: K^-1 is read inside its lower triangle below N only, X and alpha below row N only, whatever ldk is.  Found: no NaN in
  any output with NaN everywhere else, at ldk = Np and Np + 2;
* predicted: the clip sits at floor_ with the noise added after it, the keep indicator and kappa follow the same side.  Found: so it
  is - the clipped variances equal floor_ [+ noise] under another K^-1 to the bit, and the adjoint of a clipped query does not move;
* predicted: a rank-1 and a zero S go through the zero-pivot column of mm_chol, a negative in_scale through the scaling of S, dq and
  xcov with its sign.  Found: all within the bars;
* predicted, not known: NQ follows 2 cus / (G U) with the cap and R as `moments_form` restates it.  Found: every GPKMM line equals
  the mirror's (cus = 256), and the caps 1, 2, 3, 4 and every query served alone change no bit.
All 113 tests pass on the unchanged kernels; the library is unchanged but for the GPKMM log line.

Measured on an MI355X, e / bar per group (smallest .. largest over the group's cases; every case prints its own; xcov of a query
with S = 0 is exactly zero and left out):
* A (68 cases): mean 5.8e-5 .. 8.3e-3, cov 1.7e-6 .. 7.3e-3, xcov 2.5e-5 .. 2.3e-2 (the largest all at N = 1, P = 5);
* B (12): mean 9.0e-6 .. 2.6e-3, cov 1.5e-6 .. 1.1e-3, xcov 6.0e-4 .. 3.5e-3;
* C (18): mean 3.0e-5 .. 3.8e-3, cov 5.6e-7 .. 2.2e-3, xcov 7.9e-5 .. 2.7e-3, dXq 1.7e-6 .. 1.7e-3, dSq 5.3e-7 .. 1.5e-3;
* D (12): traj 1.4e-4 .. 8.4e-2, Sigma 1.7e-6 .. 1.4e-1 (a few roundings on an nx x nx composition: the sharpest bars), mean 1.4e-4
  .. 2.0e-3, cov 1.8e-6 .. 5.8e-4, xcov 7.7e-5 .. 4.7e-3, dU 3.1e-6 .. 1.7e-4, dx0 5.7e-7 .. 8.3e-4, dSigma0 1.6e-6 .. 1.2e-3.
The bars are worst-case first-order bounds on absolute values (every summand taken to round the same way through the longest
chain), which is why random rounding stays so far below them; plain fp64 NumPy uses at most 0.021 of them on the query and adjoint
cases and 0.143 on the chains, and a lost tile, row block, slot or query group moves an output by at least 1.1e4 of them
(tests/test_moments_refs.py).  The whole file takes 13 s on the GPU machine, host references included (slowest: N = 3009, 1.9 s).

The same tests against eight deliberately wrong builds of gpk_moments.hip made on a scratch copy (arithmetic or a loop bound only,
nothing more read), each run once; tests failed, and the largest e / bar of the cases over their bar:
1  `first` never cleared: 24 case tests - every case in which a workgroup walks a second tile: N = 1985 and 3009 (A, B, C, D: 4.4e8
   ..) and every batch of B >= 2 models, whose off-diagonal pairs have 4 tiles for 3 workgroups at N = 65 (.. 6.3e11); nothing else;
2  `wgt` 1 on off-diagonal tiles: 104 - every case with N > 64 (5.9e8 .. 9.7e10); the 9 that pass have one tile (N <= 64) or are
   the sequence and refusal tests, which compare bits;
3  the flush of the last chunk dropped: all 113, by the NaN that debug_fill leaves in the slots never written;
4  `r1` one short in the split kernels: 87 - every case with NQ > 1, by the NaN of each group's last query; the 26 that pass have
   NQ = 1 (moments_query_groups = 1, R = 1, G U >= 512);
5  `floor_` replaced by 0: 8 - the five clip cases and the three cases whose smallest E[v] is negative (1.1e10 .. 7.2e11);
6  the noise added inside the clip: 1 - the clip case with var_includes_noise (8.6e10);
7  `kappa` ignoring keepF: 2 - the two clip cases of the adjoint (3.6e9, 1.1e11, and the bits that must not move do);
8  the row-vector slot a a + 2 b read as a a + b (a slot that stays inside the B B slots: 2 u would leave them from B = 2
   on): 17 - every batch case of B >= 2 in B, C and D (3.3e8 .. 4.6e11); B = 1 and every single-model case pass.
"""
import ctypes as C
import sys

import numpy as np
import pytest

import test_moments_refs as R
from test_moments_refs import GROUPS, SEQUENCE, case_id, case_operands, chain_operands, padded, reference

pytestmark = pytest.mark.gpu

GUARD = 512               # fp64 elements of NaN before and behind every buffer: 4 KiB


@pytest.fixture(scope="module")
def be():
    from unmanned_aerial_vehicles_amd.device import Backend
    b = Backend(0).set_options(gram_log=1, debug_fill=1)
    yield b
    b.lib.gpk_destroy(b.h)


def _lib():
    from unmanned_aerial_vehicles_amd import _lib as lib
    return lib


def mm_lines(capfd):
    """(the words of the GPKMM lines written to stderr since the last call, the CU count they give)."""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    lines = [ln.split()[1:] for ln in cap.err.splitlines() if ln.startswith("GPKMM ")]
    cus = {int(w[3:]) for ln in lines for w in ln if w.startswith("cus")}
    assert len(cus) <= 1
    return lines, (cus.pop() if cus else None)


def guarded(be, a):
    """(the whole NaN buffer, a view holding a): 4 KiB of NaN before and behind."""
    import torch
    a = np.array(a, dtype=np.float64)
    buf = torch.full((a.size + 2 * GUARD,), float("nan"), dtype=torch.float64, device=be.device)
    view = buf[GUARD:GUARD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return buf, view


def guards_intact(pairs):
    import torch
    for buf, view in pairs:
        lo = (view.data_ptr() - buf.data_ptr()) // 8
        hi = lo + view.numel()
        assert GUARD <= lo and hi + GUARD <= buf.numel()
        if not (bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[hi:]).all())):
            return False
    return True


def host_out(shape):
    """A NaN host output between two NaN guards: (buffer, view)."""
    n = int(np.prod(shape))
    buf = np.full(n + 2 * GUARD, np.nan)
    return buf, buf[GUARD:GUARD + n].reshape(shape)


def host_guards_intact(buf, view):
    return bool(np.isnan(buf[:GUARD]).all() and np.isnan(buf[GUARD + view.size:]).all())


_dev = {}


def dev_case(be, c, kscale=1.0):
    """The device operands of a case, once: per model guarded views of X (N x D), alpha (N x P) and the K^-1 image (Np x ldk)."""
    key = (c._replace(group="", entry="", cap=0, null="", clip=0, H=0, rows="", s0=0, qn=0), kscale)
    if key not in _dev:
        o = case_operands(c)
        d = dict(bufs=[], X=[], alpha=[], Kinv=[])
        for b in range(c.B):
            for k, a in (("X", o["X"][b]), ("alpha", o["alpha"][b]), ("Kinv", R.kinv_device_image(c, b) * kscale)):
                buf, view = guarded(be, a)
                d["bufs"].append((buf, view))
                d[k].append(view)
        _dev[key] = d
    return _dev[key]


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def out_shapes(c):
    NO, nu = c.B * c.P, c.D - c.nx
    if c.entry in ("query", "vjp"):
        s = dict(mean=(c.R, NO), cov=(c.R, NO, NO), xcov=(c.R, NO, c.D))
        if c.entry == "vjp":
            s.update(dXq=(c.R, c.D), dSq=(c.R, c.nx, c.nx))
        return s
    s = dict(traj=(c.H + 1, c.R, c.nx), Sigma=(c.H + 1, c.R, c.nx, c.nx), mean=(c.H, c.R, NO), cov=(c.H, c.R, NO, NO), xcov=(c.H, c.R, NO, c.D))
    if c.entry == "chain_grad":
        s.update(dU=(c.R, c.H, nu), dx0=(c.R, c.nx), dSigma0=(c.R, c.nx, c.nx))
    return s


def case_floor(c):
    return R.chain_host(c)[1] if c.H else reference(c)["_floor"]


OWN = object()            # the case's own Sq


def invoke(be, c, d, out, floor, Xq=None, Sq=OWN, **kw):
    """One call of the case's entry into the host outputs `out` ({name: (buffer, view)}); Xq, Sq replace the case's queries (Sq None:
    a null pointer); kw replaces arguments (N, D, P, B, nx, Np, ldk, M, H, ls, sf2, scale, shift, coord: values; X, alpha, Kinv, queries,
    mean, noise, x0: None for a null pointer).  Returns the status."""
    lib, h = be.lib, be.h
    o = case_operands(c)
    keep = []                                          # (host arrays must outlive the call)

    def arr(a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a
    N, D, P, B, nx = (kw.get(k, getattr(c, k)) for k in ("N", "D", "P", "B", "nx"))
    Np = kw.get("Np", padded(c.N))
    ldk = kw.get("ldk", padded(c.N) + c.pad)
    ls = arr(kw.get("ls", o["ls"]))
    sf2 = arr(kw.get("sf2", o["sf2"]))
    ym, ys, kss, noise = arr(o["ym"]), arr(o["ys"]), arr(o["kss"]), arr(o["noise"])
    ptrs = {}
    for k in ("X", "alpha", "Kinv"):
        if c.multi:
            vals = [t.data_ptr() for t in d[k]] + [0] * max(0, B - c.B)
            if k in kw:
                vals[0] = 0                              # (a null model pointer)
            ptrs[k] = (C.c_void_p * len(vals))(*vals)
            if kw.get(k + "s", 1) is None:
                ptrs[k] = None
        else:
            ptrs[k] = None if k in kw else C.c_void_p(d[k][0].data_ptr())
    if c.multi:
        shift = kw["shift"] if "shift" in kw else (o["shift"] if c.scaler else None)
        scale = kw["scale"] if "scale" in kw else (o["scale"] if c.scaler else None)
        shift, scale = (None if a is None else vp(arr(a)) for a in (shift, scale))
        model = (B, ptrs["X"], ptrs["alpha"], N, D, vp(ls), vp(sf2), vp(ym), vp(ys), ptrs["Kinv"], Np, ldk, vp(kss), float(floor),
                 int(c.noisy), None if "noise" in kw else vp(noise))
    else:
        model = (ptrs["X"], ptrs["alpha"], N, D, P, vp(ls), float(sf2[0]), vp(ym), vp(ys), ptrs["Kinv"], Np, ldk, float(kss[0]), float(floor),
                 int(c.noisy), float(noise[0]))
    O = lambda k: None if (k in kw and kw[k] is None) or out[k][1].size == 0 else vp(out[k][1])
    be.bind_stream()
    if c.entry in ("query", "vjp"):
        xq = arr(o["Xq"] if Xq is None else Xq)
        sq = None if (Sq is None or (Sq is OWN and not c.sq)) else arr(o["Sq"] if Sq is OWN else Sq)
        M = kw.get("M", len(xq))
        tail = (nx,) + ((shift, scale) if c.multi else ()) + (None if "queries" in kw else vp(xq), vp(sq), M, O("mean"), O("cov"), O("xcov"))
        if c.entry == "vjp":
            sd = R.seeds_of(c)
            tail += tuple(vp(arr(sd[k])) if sd[k] is not None else None for k in ("gmean", "gcov", "gxcov")) + (O("dXq"), O("dSq"))
        fn = getattr(lib, ("gpk_moments_vjp_host" if c.entry == "vjp" else "gpk_moments_host") + ("_multi" if c.multi else ""))
        return fn(h, *model, *tail)
    co = chain_operands(c)
    rows = co["rows"]
    nu = D - nx
    Uarr = arr(co["U"]) if nu > 0 else None
    coord = kw.get("coord", co["coord"])
    head = ((nx, (C.c_int * len(coord))(*coord), shift, scale) if c.multi else ())
    tail = head + (None if "x0" in kw else vp(arr(co["x0"])), kw.get("x0_rows", rows[0]), vp(Uarr), rows[1], vp(arr(co["lin"])),
                   vp(arr(co["Sigma0"])) if c.s0 else None, rows[2], vp(arr(co["Q"])) if c.qn else None, kw.get("R", c.R), kw.get("H", c.H),
                   O("traj"), O("Sigma"), O("mean"), O("cov"), O("xcov"))
    if c.entry == "chain_grad":
        tail += (vp(arr(co["gx"])), vp(arr(co["gS"])), O("dU"), O("dx0"), O("dSigma0"))
    fn = getattr(lib, ("gpk_propagate_mm_grad_host" if c.entry == "chain_grad" else "gpk_propagate_mm_host") + ("_multi" if c.multi else ""))
    return fn(h, *model, *tail)


def settled(be, rc, who):
    """Behind an accepted call: the stream is drained.  A refusal (GPK_BAD_ARG: a mistake in the test's arguments, nothing was
    launched) fails the test; any other status - a failed launch, a device fault - ends the session: nothing more is started on
    the device."""
    if rc == 0:
        rc = be.lib.gpk_synchronize(be.h)
    msg = be.lib.gpk_last_error(be.h).decode() if rc else ""
    assert rc != _lib().GPK_BAD_ARG, f"{who}: refused: {msg}"
    if rc:
        pytest.exit(f"{who}: status {rc}: {msg}", returncode=3)


def expected_lines(c, cus):
    return R.chain_lines(c, cus) if c.H else R.case_lines(c, cus)


def run_once(be, capfd, c, kscale=1.0, Xq=None, Sq=OWN, lines=True):
    """One call into NaN outputs: status 0, the GPKMM lines of the mirror, every output written, the outputs' guards still NaN.
    Returns {output: host array}."""
    d = dev_case(be, c, kscale)
    shapes = out_shapes(c)
    if Xq is not None:
        shapes = {k: (len(Xq),) + s[1:] for k, s in shapes.items()}
    out = {k: host_out(s) for k, s in shapes.items()}
    mm_lines(capfd)
    be.set_options(moments_query_groups=c.cap)
    try:
        rc = invoke(be, c, d, out, case_floor(c), Xq, Sq)
    finally:
        be.set_options(moments_query_groups=0)
    settled(be, rc, case_id(c))
    got, cus = mm_lines(capfd)
    if lines:
        want = expected_lines(c, cus)
        assert got == want, (got, want)
    res = {}
    for k, (buf, view) in out.items():
        assert host_guards_intact(buf, view), f"nothing before or behind {k} may be written"
        assert not np.isnan(view).any(), f"every entry of {k} is written, from nothing that is NaN"
        res[k] = view
    return res


_got = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def run(be, capfd, c):
    """The case twice with identical bits, the operands' guards still NaN; cached."""
    if c not in _got:
        r0, r1 = run_once(be, capfd, c), run_once(be, capfd, c)
        for k in r0:
            assert np.array_equal(bits(r0[k]), bits(r1[k])), f"{k}: two runs must give identical bits"
        assert guards_intact(dev_case(be, c)["bufs"])
        _got[c] = r0
    return _got[c]


def symmetric(got, names):
    for k in names:
        if k in got:
            assert np.array_equal(bits(got[k]), bits(np.swapaxes(got[k], -1, -2))), f"{k}: both triangles come from one sum"


def check_case(be, capfd, c):
    """Every check of a query or vjp case; returns {output: (e / bar, e, bar)} at the worst entry."""
    got = run(be, capfd, c)
    w = R.worst(c, got)
    print(f"{case_id(c)}: " + ", ".join(f"{k} e / bar {v[0]:.1e} (e {v[1]:.2e}, bar {v[2]:.2e})" for k, v in w.items()))
    symmetric(got, ("cov", "dSq"))
    ref = reference(c)
    if c.sq:
        assert np.array_equal(got["xcov"][0], np.zeros_like(got["xcov"][0])), "row 0 has S = 0: xcov is exactly zero"
    assert np.array_equal(got["xcov"][:, :, c.nx:], np.zeros_like(got["xcov"][:, :, c.nx:]))
    if c.entry == "vjp":        # mean, cov, xcov of a vjp call have the bits of the forward call
        fwd = run(be, capfd, c._replace(entry="query", null=""))
        for k in ("mean", "cov", "xcov"):
            assert np.array_equal(bits(got[k]), bits(fwd[k])), f"{k}: the vjp entry keeps the forward call's bits"
    if c.clip:
        # another K^-1 (times KSCALE = 1 + 2^-20: the reference's E[v] under it stays on its side of floor_, 1e5 bars away, and moves
        # by more than 100 bars - all three asserted in tests/test_moments_refs.py, test_clip_gap) must leave the variance of the clipped models - and what their clip passes back - with the same bits
        keep = ref["_keep"]
        assert keep.any() and (~keep).any()
        other = run_once(be, capfd, c, kscale=R.KSCALE)
        for r in range(c.R):
            for o in range(c.B * c.P):
                b = o // c.P if c.B > 1 else 0
                same = got["cov"][r, o, o] == other["cov"][r, o, o]
                assert same == (not keep[r, b]), (r, o, "the clipped variance is floor_ [+ noise] whatever K^-1 is, the others move")
            if c.entry == "vjp":
                moved = not (np.array_equal(bits(got["dXq"][r]), bits(other["dXq"][r])) and np.array_equal(bits(got["dSq"][r]), bits(other["dSq"][r])))
                assert moved == bool(keep[r].any()), (r, "a clipped variance contributes exactly nothing to the adjoint")
    for k, v in w.items():
        assert v[0] <= 1.0, (k, v)
    return w


# ---- A .. C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUPS["A"], ids=case_id)
def test_forward(be, capfd, c):
    check_case(be, capfd, c)


@pytest.mark.parametrize("c", GROUPS["B"], ids=case_id)
def test_forward_batch(be, capfd, c):
    check_case(be, capfd, c)


@pytest.mark.parametrize("c", GROUPS["C"], ids=case_id)
def test_adjoint(be, capfd, c):
    check_case(be, capfd, c)


def test_query_groups_change_no_bit(be, capfd):
    """The same case under every cap, and every query alone, has the bits of the default launch."""
    base = [c for c in GROUPS["A"] if c.R == 5 and c.P == 2 and c.cap == 3][0]
    want = run(be, capfd, base)
    for cap in (1, 2, 4, 0):
        got = run(be, capfd, base._replace(cap=cap))
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), (cap, k)
    o = case_operands(base)
    for r in range(base.R):
        alone = run_once(be, capfd, base, Xq=o["Xq"][r:r + 1], Sq=o["Sq"][r:r + 1], lines=False)
        for k in want:
            assert np.array_equal(bits(alone[k][0]), bits(want[k][r])), (r, k)


# ---- D: the chains ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUPS["D"], ids=case_id)
def test_chain(be, capfd, c):
    got = run(be, capfd, c)
    w = R.check_chain(c, got)
    print(f"{case_id(c)}: " + ", ".join(f"{k} e / bar {v[0]:.1e} (e {v[1]:.2e}, bar {v[2]:.2e})" for k, v in w.items()))
    symmetric(got, ("cov", "Sigma", "dSigma0"))
    co = chain_operands(c)
    U = np.broadcast_to(co["U"], (c.R, c.H, c.D - c.nx))
    q = c._replace(entry="query", H=0)
    for h in range(c.H):       # the stage outputs have the bits of the query entry on the same rows
        Xq = np.concatenate([got["traj"][h], U[:, h]], axis=1)
        d = dev_case(be, q)
        out = {k: host_out(s) for k, s in out_shapes(q).items()}
        settled(be, invoke(be, q, d, out, case_floor(c), Xq, got["Sigma"][h]), case_id(q))
        for k in ("mean", "cov", "xcov"):
            assert np.array_equal(bits(out[k][1]), bits(got[k][h])), (h, k, "a stage's outputs have the bits of the query entry")
    if c.entry == "chain_grad":
        fwd = run(be, capfd, c._replace(entry="chain"))
        for k in fwd:
            assert np.array_equal(bits(got[k]), bits(fwd[k])), f"{k}: the gradient entry keeps the chain's bits"
    for k, v in w.items():
        assert v[0] <= 1.0, (k, v)


# ---- E: one handle -----------------------------------------------------------------------------------------------------------------
def test_sequence_on_one_handle(be, capfd):
    """Six calls of different entries and sizes on one new handle: the scratch block grows and shrinks in use; under debug_fill only
    the bytes asked for are NaN, so a sum that read a slot of an earlier call would give other bits than the case's own run."""
    from unmanned_aerial_vehicles_amd.device import Backend
    seq = SEQUENCE + [GROUPS["D"][3], GROUPS["D"][8]]
    alone = [run(be, capfd, c) for c in seq]
    be2 = Backend(0).set_options(gram_log=1, debug_fill=1)
    try:
        for c, want in zip(seq, alone):
            got = run_once(be2, capfd, c)
            for k in want:
                assert np.array_equal(bits(got[k]), bits(want[k])), (case_id(c), k)
    finally:
        be2.lib.gpk_destroy(be2.h)


def test_refusals(be, capfd):
    from unmanned_aerial_vehicles_amd import _lib
    one, multi = GROUPS["A"][2], GROUPS["B"][10]
    chain, mchain = GROUPS["D"][2], GROUPS["D"][8]
    Np = padded(one.N)
    ls_of = lambda c, x: np.where(np.arange(c.B * c.D).reshape(c.B, c.D) == c.D - 1, x, case_operands(c)["ls"])
    calls = []
    for c in (one, multi, chain, mchain):
        Npc = padded(c.N)
        calls += [(c, "N = 0", dict(N=0)), (c, "D = 0", dict(D=0)), (c, "D = 17", dict(D=17, ls=np.ones((c.B, 17)))),
                  (c, "Np != gpk_padded(N)", dict(Np=Npc + 128, ldk=Npc + 128)), (c, "ldk < Np", dict(ldk=Npc - 2)),
                  (c, "a zero length-scale", dict(ls=ls_of(c, 0.0))), (c, "a negative length-scale", dict(ls=ls_of(c, -1.0))),
                  (c, "a NaN length-scale", dict(ls=ls_of(c, np.nan))), (c, "sf2 = 0", dict(sf2=np.zeros(c.B))),
                  (c, "X null", dict(X=None)), (c, "alpha null", dict(alpha=None)), (c, "K^-1 null", dict(Kinv=None)),
                  (c, "batched mode", dict(batch=2))]
    for c in (one, multi):
        calls += [(c, "nx = 0", dict(nx=0)), (c, "nx > D", dict(nx=c.D + 1)), (c, "M = 0", dict(M=0)), (c, "M = 33", dict(M=33)),
                  (c, "Xq null", dict(queries=None)), (c, "mean null", dict(mean=None))]
    calls += [(one, "P = 0", dict(P=0)), (one, "P = 17", dict(P=17)), (chain, "P > D", dict(P=chain.D + 1)),
              (multi, "B = 0", dict(B=0)), (multi, "B = 9", dict(B=9)), (multi, "in_scale alone", dict(shift=None)),
              (multi, "in_scale zero", dict(scale=np.zeros(multi.D))), (multi, "the model pointers null", dict(Xs=None)),
              (mchain, "nx below the number of outputs", dict(nx=mchain.B - 1)), (mchain, "coord out of range", dict(coord=[0, mchain.nx])),
              (mchain, "coord repeated", dict(coord=[1, 1])), (chain, "R = 0", dict(R=0)), (chain, "R = 33", dict(R=33)),
              (chain, "H = 0", dict(H=0)), (chain, "x0 null", dict(x0=None)), (chain, "x0 with two rows", dict(x0_rows=2)),
              (mchain, "traj null", dict(traj=None))]
    for c, what, kw in calls:
        d = dev_case(be, c)
        out = {k: host_out(s) for k, s in out_shapes(c).items()}
        mm_lines(capfd)
        batch = kw.pop("batch", 0)
        if batch:
            assert be.lib.gpk_batch_begin(be.h, batch) == 0
        rc = invoke(be, c, d, out, case_floor(c), **kw)
        msg = be.lib.gpk_last_error(be.h).decode()
        if batch:
            assert be.lib.gpk_batch_end(be.h) == 0
        assert rc == _lib.GPK_BAD_ARG and msg.startswith("bad argument"), (case_id(c), what, rc, msg)
        be.sync()
        assert mm_lines(capfd)[0] == [], "a refused call must not launch"
        assert all(np.isnan(buf).all() for buf, _ in out.values()), (case_id(c), what)
        # ... and the handle still serves: the case's own call has the bits of its first run
        if what in ("ldk < Np", "batched mode", "coord repeated", "M = 33"):
            want, again = run(be, capfd, c), run_once(be, capfd, c)
            for k in want:
                assert np.array_equal(bits(again[k]), bits(want[k])), (case_id(c), what, k)
    for c in (one, multi, chain, mchain):
        again, want = run_once(be, capfd, c), run(be, capfd, c)
        for k in want:
            assert np.array_equal(bits(again[k]), bits(want[k])), (case_id(c), k)
