"""Every launch form of the large-batch derivative kernels (K8) through their five C entries - gpk_jac.hip:
predict_mean_grad_kernel<D4, PS>, predict_mean_grad_multi_kernel<D4, BS>, var_grad_kernel<D4> and their three reductions;
gpk_hess.hip: predict_mean_hess_kernel<D4, PS> with its row blocks, predict_mean_hess_multi_kernel<D4, BS> and two reductions - on
operands the test builds itself, against the extended-precision reference, the launch-rule mirror and the bars of
tests/test_deriv_refs.py:

A  gpk_predict_mean_grad: the 16 (d4, ps) pairs, D in {1, 4, 5, 8, 9, 12, 13, 16}, P in {1, 2, 3, 4, 5 (3 + 2), 7 (4 + 3), 9, 13 (4, 4,
   4, 1), 16}, N in {1, 31, 32, 33, 127, 128, 129, 300}, M in {1, 255, 256, 257, 512, 513}, N = 16384 | 16385 at M = 1 (32- and 128-row
   chunks), M = 20000 (chunks of two staging rounds, the last round ragged), M = 65537 (two panels, the second of one query);
B  gpk_predict_mean_grad_multi: the 16 (d4, bs) pairs, B = 1 .. 8, the same edges thinned, M = 65537;
C  gpk_predict_var_grad_inv: d4 = 1 .. 4, Np in {128, 256, 640} with N = Np and N = Np - 127, M in {1, 127, 128, 129, 300}, ldw = Np and
   Np + 2, var NULL and not, the clip (the clipped entries equal floor_ exactly, dvar is still the unclipped gradient), Np = 2304
   (W NaN beyond the zero band), and N = 640, M = 29057 (chunks of two 64-row rounds; the smallest Np whose N M reaches 1.9e7);
D  gpk_predict_mean_hess: the seven forms, D in {1, 2, 3, 4, 5, 8, 9, 12, 13, 14, 16} (row blocks partly filled at D = 9, 14 and empty
   at D = 13), M = 8192 with P = D = 16 (capS: one chunk of three rounds), M = 15105 (the reduced panel of 15104 and one query);
E  gpk_predict_mean_hess_multi: the seven forms, B = 1 .. 8 with odd B above D = 4, D in {1, 4, 5, 8, 9, 12, 13, 15, 16} (all five row
   blocks of d4 = 4, the empty [14, 16) at D = 13), M = 48897 at B = 5, D = 16 (the reduced panel of 48896 and one query);
F  six calls of different entries on one new handle (the scratch under debug_fill), and the refusals.

A fresh handle with the options `gram_log` (every call's GPKDERIV lines are asserted against `deriv_form`) and `debug_fill` (the
chunks' partial sums start as NaN: a slot read before it is written shows).  X, alpha, Xq, W and the variance gradient's work
panels are views into NaN-filled device buffers with 4 KiB of NaN before and behind; W is exactly zero above the diagonal inside
the band gpk_trtri zeroes and NaN beyond it and in the pitch columns; outputs start as NaN between two such guards, and every element of a buffer outside its view is guard.  Every
case runs twice and must give identical bits; its GPKDERIV lines equal the mirror's; every output is within its bar of the
reference; the guards are still NaN; Hessians are symmetric to the bit; e / bar is printed per output.  A case with more queries
than one period (768; vargrad 384) repeats its first period: the first period of every panel is compared with the reference, and
every later query of the panel must have the bits of its copy in that first period - compared on the device.  X, alpha and Xq of
the cases marked off8 lie at addresses that are 8- but not 16-byte aligned: the four mean entries read them with scalar 8-byte
loads only (read from the kernels: `X[(jb + j) * D + c]`, `alpha[...]`, `Xq[qm * D + d]`; include/gpk.h asks for no alignment
there); gpk_predict_var_grad_inv goes through the tile GEMMs and keeps 16-byte alignment.

Predicted from reading the code, and found:
* predicted: the index arithmetic of all ten kernels is right - the staging loops stop at min(N, n0 + chunk), every store is masked
  by qm < M, p0 + p < P (b0 + b < B) and d < D, the reductions read the slots tri(d) + e, d < D, and tri(D) alone, so the slots of an
  empty or partly filled row block are never read - and every case passes on the unchanged kernels.  Found: so it is - all 77
  cases pass; the library is unchanged but for the GPKDERIV log line;
* predicted: W is multiplied only inside its lower triangle and the zero band (both GEMMs of gpk_predict_var_grad_inv run with
  k_super, whose ranges end within GPK_ZERO_BAND_TILES tiles of the diagonal), and K*'s padding is written before it is read.
  Found: no NaN in any output at Np = 2304 or under NaN-filled work panels;
* predicted: var_grad_kernel adds the first N rows of V only, so on a dense random W whose rows N .. Np - 1 are not zero left of
  column N `var` would not be kss - |W k*|^2.  Not run: such a W is no inverse factor (include/gpk.h: W from gpk_trtri), so the
  operands keep that block zero (tests/test_deriv_refs.py) and the literal formula holds;
* predicted, not known: a query's var and dvar do not depend on its tile column (one thread per column in var_grad_kernel, one
  k-order per element in the GEMMs).  Found: so it is - all 28673 later queries of N = 640, M = 29057 have the bits of their copies
  in the first 384, and the test asserts it as it does for the other entries;
* predicted: the four mean entries take X, alpha and Xq at any 8-byte boundary.  Found: the ten off8 cases pass, same bars.

Measured on an MI355X, e / bar per group (smallest .. largest over the group's cases; every case prints its own):
* A: dmean 1.9e-5 (N = 16384, M = 1) .. 5.4e-2 (N = 33, D = 9, P = 9);   B: dmean 3.8e-3 .. 8.9e-2 (N = 1);
* C: var 1.1e-6 (Np = 2304) .. 2.9e-3 (N = 1), dvar 9.9e-7 (Np = 2304) .. 8.3e-2 (N = 1);
* D: hess 5.4e-3 .. 6.9e-2 (M = 15105);   E: hess 3.6e-3 .. 7.7e-2 (N = 33, D = 12, B = 5).
The bars are worst-case first-order bounds on absolute values; plain fp64 NumPy uses at most 0.14 of them (tests/test_deriv_refs.py).
The whole file takes 12 s on the GPU machine, host references included (slowest: the capS case 2.8 s, Np = 2304 1.2 s).

The same cases against seven deliberately wrong builds of gpk_jac.hip / gpk_hess.hip made on a scratch copy (arithmetic or a loop
bound only, no address moved, no barrier removed, nothing more read), each run once; tests failed, and e / bar of the cases over
their bar:
1  every reduction stops one chunk early: 62 case tests - every case with more than one chunk in some panel (3.1e6 at Np = 2304 ..
   2.8e13); the 15 that pass have one chunk in every panel (N <= 32, or N <= 128 with 128-row chunks, or the Hessian's capS);
2  the second staging round is skipped: 3 tests, exactly the cases whose chunks have one - A N = 1000, M = 20000 (dmean 1.7e12), C
   N = 640, M = 29057 (var 1.9e10, dvar 9.1e9) and D M = 8192 (hess 6.4e12);
3  the last live slot of a group that is not full is not written (the staging mask itself cannot change a written result: a slot
   past P or B is stored nowhere): 15 case tests - every P or B that is no multiple of ps or bs (P = 5, 7, 13; B = 5, 7; odd B
   above D = 4, B = 1 included) - by the NaN left in the output, and the sequence and the refusals' accepted calls with them;
4  row block [8, 12) starts at 9: 2 tests, the two D cases of d4 = 3 (D = 9, 12), by the NaN of row 8;
5  S_p subtracted before the scaling in the multi reduction: all 15 E cases (hess 5.8e12 .. 3.6e14), nothing else;
6  y_std[0] for every output: 51 case tests - every A, B, D, E case with more than one output or model (1.1e12 .. 8.2e13); those
   with one pass;
7  128-row chunks everywhere: 55 case tests, every mean case with M <= 512 and N <= 16384, all by their GPKDERIV line (gran, s, chunk) -
   the values stay within their bars, as they must.
"""
import sys

import numpy as np
import pytest

import test_deriv_refs as R
from test_deriv_refs import GROUPS, SEQUENCE, case_bars, case_form, case_id, case_lines, case_operands, deriv_reference, fast_hp, outputs_of, padded, ratio

pytestmark = pytest.mark.gpu

GUARD = 512               # fp64 elements of NaN before and behind every device buffer: 4 KiB


@pytest.fixture(scope="module")
def be():
    from unmanned_aerial_vehicles_amd.device import Backend
    b = Backend(0).set_options(gram_log=1, debug_fill=1)
    yield b
    b.lib.gpk_destroy(b.h)


def deriv_lines(capfd):
    """The words of the GPKDERIV lines (option gram_log) written to stderr since the last call."""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    return [ln.split()[1:] for ln in cap.err.splitlines() if ln.startswith("GPKDERIV ")]


def guarded_empty(be, n, off=0):
    """(the whole NaN buffer, a view of n fp64 elements inside it): 4 KiB of NaN before and behind (off = 1: 8 bytes more on either
    side, the view starts 8 bytes past a 16-byte boundary).  Everything outside the view is guard: `guards_intact`."""
    import torch
    buf = torch.full((n + 2 * (GUARD + off),), float("nan"), dtype=torch.float64, device=be.device)
    view = buf[GUARD + off:GUARD + off + n]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 * off
    return buf, view


def guarded(be, a, off=0):
    import torch
    a = np.array(a, dtype=np.float64)      # (a copy: the cached operands are read-only)
    buf, view = guarded_empty(be, a.size, off)
    view = view.view(a.shape)
    view.copy_(torch.from_numpy(a))
    return buf, view


def guards_intact(pairs):
    """Every element of every buffer outside its view - from the buffer's first element up to the view, and from the element
    right behind the view to the buffer's last - is still NaN.  pairs: (buffer, view)."""
    import torch
    for buf, view in pairs:
        lo = (view.data_ptr() - buf.data_ptr()) // 8
        hi = lo + view.numel()
        assert GUARD <= lo and hi + GUARD <= buf.numel()
        if not (bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[hi:]).all())):
            return False
    return True


_dev = {}


def dev_case(be, c):
    """The operands of a case on the device, once: guarded views of X, alpha (N x P | B), Xq (all M queries: the first period repeated),
    W (Np x ldw) and the work panels; the host arrays ls, sf2, ys."""
    import torch
    if c in _dev:
        return _dev[c]
    o = case_operands(c)
    d = dict(bufs=[])

    def put(key, a, off=c.off):
        buf, view = guarded(be, a, off)
        d["bufs"].append((buf, view))
        d[key] = view

    put("X", o["X"][0])
    put("alpha", np.concatenate(o["alpha"], axis=1))
    first = torch.from_numpy(np.array(o["Xq"])).to(be.device)
    buf, view = guarded_empty(be, c.M * c.D, c.off)
    view = view.view(c.M, c.D)
    view.copy_(first[torch.arange(c.M, device=be.device) % R.period(c)])
    d["bufs"].append((buf, view))
    d["Xq"] = view
    d["ls"] = np.ascontiguousarray(np.stack(o["ls"]))
    d["sf2"] = np.array(o["sf2"])
    d["ys"] = np.ascontiguousarray(o["ys"])
    if c.entry == "vargrad":
        put("W", R.w_device_image(c), 0)
        Np = padded(c.N)
        buf, view = guarded_empty(be, 3 * Np * padded(c.M))
        d["bufs"].append((buf, view))
        d["work"] = view
        d["kss"] = o["kss"][0]
    _dev[c] = d
    return d


def out_shapes(c):
    return dict(dmean=(c.M, c.P, c.D), hess=(c.M, c.P, c.D, c.D), var=(c.M,), dvar=(c.M, c.D))


def nan_outputs(be, c):
    """{output: (buffer, view)} - NaN, with the guards."""
    res = {}
    for k in outputs_of(c):
        buf, view = guarded_empty(be, int(np.prod(out_shapes(c)[k])))
        res[k] = (buf, view.view(out_shapes(c)[k]))
    return res


def invoke(be, c, d, out, **kw):
    """One call of the case's entry; kw replaces arguments (N, D, P, M, Np, ldw, ls: values; X, alpha, Xq, W, work, ys, sf2v, res: None
    for a null pointer).  Returns the status."""
    from unmanned_aerial_vehicles_amd._lib import dev_ptr as p, host_ptr as hp
    lib, h = be.lib, be.h
    N, D, P, M = (kw.get(k, getattr(c, k)) for k in "NDPM")
    ls = np.ascontiguousarray(kw.get("ls", d["ls"]))
    X, alpha, Xq = (p(d[k]) if kw.get(k, 1) is not None else None for k in ("X", "alpha", "Xq"))
    ys = hp(d["ys"]) if kw.get("ys", 1) is not None else None
    main = None if kw.get("res", 1) is None else p(out[outputs_of(c)[-1]][1])
    be.bind_stream()
    if c.entry == "vargrad":
        Np = kw.get("Np", padded(c.N))
        W, work = (p(d[k]) if kw.get(k, 1) is not None else None for k in ("W", "work"))
        var = p(out["var"][1]) if c.var else None
        return lib.gpk_predict_var_grad_inv(h, X, N, D, hp(ls), float(d["sf2"][0]), W, Np, kw.get("ldw", Np + c.pad), Xq, M, float(d["kss"]),
                                            R.SR.FLOOR, work, var, main)
    if c.entry in ("grad", "hess"):
        fn = lib.gpk_predict_mean_grad if c.entry == "grad" else lib.gpk_predict_mean_hess
        return fn(h, X, alpha, N, D, P, hp(ls) if kw.get("ls", 1) is not None else None, float(d["sf2"][0]), ys, Xq, M, main)
    fn = lib.gpk_predict_mean_grad_multi if c.entry == "grad_multi" else lib.gpk_predict_mean_hess_multi
    sf2 = hp(d["sf2"]) if kw.get("sf2v", 1) is not None else None
    return fn(h, X, alpha, N, D, P, hp(ls) if kw.get("ls", 1) is not None else None, sf2, ys, Xq, M, main)


def run_once(be, capfd, c):
    """One call into NaN outputs: status 0, the GPKDERIV lines of the mirror, every output written from nothing that is NaN, the
    guards behind the outputs still NaN.  Returns {output: device tensor}."""
    import torch
    d = dev_case(be, c)
    out = nan_outputs(be, c)
    deriv_lines(capfd)
    rc = invoke(be, c, d, out)
    if rc == 0:
        rc = be.lib.gpk_synchronize(be.h)
    if rc:                      # a failed launch or a device fault: nothing more is started on the device
        pytest.exit(f"{c.entry} on {case_id(c)}: status {rc}: {be.lib.gpk_last_error(be.h).decode()}", returncode=3)
    lines, want = deriv_lines(capfd), case_lines(c)
    assert lines == want, (lines, want)
    res = {}
    for k, (buf, view) in out.items():
        assert guards_intact([(buf, view)]), f"nothing before or behind {k} may be written"
        assert not bool(torch.isnan(view).any()), f"every entry of {k} is written, from nothing that is NaN"
        res[k] = view
    return res


_got = {}


def run(be, capfd, c):
    """The case twice with identical bits, the operands' guards still NaN; cached."""
    import torch
    if c not in _got:
        r0, r1 = run_once(be, capfd, c), run_once(be, capfd, c)
        for k in r0:
            assert torch.equal(r0[k].view(torch.int64), r1[k].view(torch.int64)), f"{k}: two runs must give identical bits"
        assert guards_intact(dev_case(be, c)["bufs"])
        del r1
        _got[c] = r0
    return _got[c]


def check_case(be, capfd, c):
    """Every check of one case; returns {output: (e / bar, e, bar)} at the worst entry.  A HIP error ends the session: nothing more
    is started on a device that has faulted."""
    try:
        return _check_case(be, capfd, c)
    except RuntimeError as e:
        if "HIP" in str(e) or "hip" in str(e):
            pytest.exit(f"{case_id(c)}: {e}", returncode=3)
        raise


def _check_case(be, capfd, c):
    import torch
    got = run(be, capfd, c)
    hp, ref, bars = fast_hp(), deriv_reference(c), case_bars(c)
    per = R.period(c)
    worst, late = {}, []
    for k in outputs_of(c):
        g = got[k]
        for pn in case_form(c):
            # the first period of the panel against the reference ...
            n = min(pn.mc, per)
            rows = (pn.m0 + np.arange(n)) % per
            head = g[pn.m0:pn.m0 + n].cpu().numpy()
            r = ratio(hp.f64(np.abs(hp.arr(head) - ref[k][1][rows])), bars[k][rows])
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            w = (float(r[i]), float(np.abs(head - ref[k][0][rows])[i]), float(bars[k][rows][i]))
            if k not in worst or w[0] > worst[k][0]:
                worst[k] = w
            # ... and every later query of the panel against its copy there, on the device
            if pn.mc > per:
                src = pn.m0 + torch.arange(pn.mc - per, device=g.device) % per
                rest = g[pn.m0 + per:pn.m0 + pn.mc]
                late.append((k, torch.equal(rest.view(torch.int64), g[src].view(torch.int64))))
    print(f"{case_id(c)}: " + ", ".join(f"{k} e / bar {w[0]:.1e} (e {w[1]:.2e}, bar {w[2]:.2e})" for k, w in worst.items()))
    for k, ok in late:
        assert ok, f"{k}: a later query must have the bits of its copy in the first period"
    if "hess" in got:
        hs = got["hess"]
        assert torch.equal(hs.view(torch.int64), hs.transpose(-1, -2).contiguous().view(torch.int64)), "both triangles come from one sum"
    if c.regime == "clip":
        var = got["var"].cpu().numpy()
        clipped = ref["_raw"] < R.SR.FLOOR
        assert clipped.any() and np.array_equal(var[clipped], np.full(int(clipped.sum()), R.SR.FLOOR)) and (var[~clipped] > R.SR.FLOOR).all()
    for k, w in worst.items():
        assert w[0] <= 1.0, (k, w)
    return worst


# ---- A .. E ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUPS["A"], ids=case_id)
def test_mean_grad(be, capfd, c):
    check_case(be, capfd, c)


@pytest.mark.parametrize("c", GROUPS["B"], ids=case_id)
def test_mean_grad_multi(be, capfd, c):
    check_case(be, capfd, c)


@pytest.mark.parametrize("c", GROUPS["C"], ids=case_id)
def test_var_grad(be, capfd, c):
    check_case(be, capfd, c)
    if not c.var:      # a NULL var changes nothing in dvar
        import torch
        dv = run(be, capfd, c._replace(var=1))["dvar"]
        assert torch.equal(dv.view(torch.int64), run(be, capfd, c)["dvar"].view(torch.int64))


@pytest.mark.parametrize("c", GROUPS["D"], ids=case_id)
def test_mean_hess(be, capfd, c):
    check_case(be, capfd, c)


@pytest.mark.parametrize("c", GROUPS["E"], ids=case_id)
def test_mean_hess_multi(be, capfd, c):
    check_case(be, capfd, c)


# ---- F: one handle -----------------------------------------------------------------------------------------------------------
def test_sequence_on_one_handle(be, capfd):
    """hess -> grad (N = 1) -> vargrad -> hess_multi -> grad_multi -> grad on one new handle: the scratch block is taken at 17 MB, then
    asked for 8 bytes, then grows and shrinks in use; under debug_fill only the bytes asked for are NaN, so a reduction that read a
    slot of an earlier call's partial sums would give other bits than the case's own run."""
    import torch
    from unmanned_aerial_vehicles_amd.device import Backend
    alone = [run(be, capfd, c) for c in SEQUENCE]
    be2 = Backend(0).set_options(gram_log=1, debug_fill=1)
    try:
        for c, want in zip(SEQUENCE, alone):
            got = run_once(be2, capfd, c)
            for k in outputs_of(c):
                assert torch.equal(got[k].view(torch.int64), want[k].view(torch.int64)), (case_id(c), k)
    finally:
        be2.lib.gpk_destroy(be2.h)


def test_refusals(be, capfd):
    import torch
    from unmanned_aerial_vehicles_amd import _lib
    g, m, v, hs, hm = GROUPS["A"][6], GROUPS["B"][6], GROUPS["C"][3], GROUPS["D"][4], GROUPS["E"][7]
    bad_ls = lambda c, x: np.where(np.arange(np.stack(case_operands(c)["ls"]).size).reshape(-1, c.D) == c.D - 1, x, np.stack(case_operands(c)["ls"]))
    wide = lambda c: np.ones((8, 17))
    calls = []
    for c in (g, m, hs, hm):
        calls += [(c, "D = 0", dict(D=0)), (c, "D = 17", dict(D=17, ls=wide(c))), (c, "N = 0", dict(N=0)), (c, "M = 0", dict(M=0)),
                  (c, "a zero length-scale", dict(ls=bad_ls(c, 0.0))), (c, "a negative length-scale", dict(ls=bad_ls(c, -1.0))),
                  (c, "X null", dict(X=None)), (c, "alpha null", dict(alpha=None)), (c, "Xq null", dict(Xq=None)), (c, "y_std null", dict(ys=None)),
                  (c, "the output null", dict(res=None))]
    calls += [(g, "P = 17", dict(P=17)), (hs, "P = 17", dict(P=17)), (g, "P = 0", dict(P=0)), (hs, "ls null", dict(ls=None))]
    for c in (m, hm):
        calls += [(c, "B = 0", dict(P=0)), (c, "B = 9", dict(P=9)), (c, "sf2 null", dict(sf2v=None)), (c, "ls null", dict(ls=None))]
    Np = padded(v.N)
    calls += [(v, "D = 0", dict(D=0)), (v, "D = 17", dict(D=17, ls=wide(v))), (v, "N = 0", dict(N=0)), (v, "M = 0", dict(M=0)),
              (v, "a zero length-scale", dict(ls=bad_ls(v, 0.0))), (v, "X null", dict(X=None)), (v, "W null", dict(W=None)),
              (v, "Xq null", dict(Xq=None)), (v, "work null", dict(work=None)), (v, "dvar null", dict(res=None)),
              (v, "Np != gpk_padded(N)", dict(Np=Np + 128, ldw=Np + 128)), (v, "Np = N", dict(Np=v.N, ldw=Np)), (v, "ldw < Np", dict(ldw=Np - 2)),
              (v, "batched mode", dict(batch=2))]
    for c, what, kw in calls:
        d = dev_case(be, c)
        out = nan_outputs(be, c)
        deriv_lines(capfd)
        batch = kw.pop("batch", 0)
        if batch:
            assert be.lib.gpk_batch_begin(be.h, batch) == 0
        rc = invoke(be, c, d, out, **kw)
        msg = be.lib.gpk_last_error(be.h).decode()
        if batch:
            assert be.lib.gpk_batch_end(be.h) == 0
        assert rc == _lib.GPK_BAD_ARG and msg.startswith("bad argument"), (c.entry, what, rc, msg)
        be.sync()
        assert deriv_lines(capfd) == [], "a refused call must not launch"
        assert all(bool(torch.isnan(buf).all()) for buf, _ in out.values()), (c.entry, what)
    # ... and the same arguments are accepted once nothing is wrong with them
    for c in (g, m, v, hs, hm):
        check_case(be, capfd, c)
