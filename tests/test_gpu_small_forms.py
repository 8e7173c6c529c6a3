"""Every launch form of the small-batch serving kernels (gpk_small.hip: small_cross_mean[_jac]_kernel, small_var[_grad]_kernel,
small_cov_kernel, small_wtv_grad_kernel, small_hess_kernel - the one-factor instantiations) through the eight one-call entries
gpk_predict_host[_multi][_cov|_grad|_hess], on operands the test builds itself - no fitted model - against the extended-precision
reference, the launch-rule mirror and the bars of tests/test_small_refs.py:

A  mean only: N in {1, 31, 32, 33, 128, 129, 1000}, D in {1, 9, 16}, M P across 64 | 128 | 256 and at 512 (finish_means in 4, 2, 1
   parts and in two passes), M = 33 and 64 (two chunks of queries);
B  mean + variance: Np = 128 (idle waves; N = Np and N = Np - 127), 640 (nine and ten chunks: one pipelined round), 1152 (two), 2176
   (136 shares: a second sum_shares round), M in {1, 16, 17, 32}, ldw = Np and Np + 2, and kss between the queries' subtracted terms:
   the clipped variances equal floor_ exactly;
C  covariance: Np in {128, 256, 384, 2176} (half a group, one, one and a half, nine with a second round at the top level), P in
   {1, 3}; symmetric to the bit; noise on the diagonal only, the pair of identical queries included;
D  gradients: mean + Jacobian at M P D = 1, 1024, 1040, 8192; all four results at Np = 128 (rc 4), 2048 (rc 2), 2176 (rc 1), M D = 512;
E  Hessian: N = 1 (three empty workgroups), 33, 129, Np = 2176 (34 rows: rounds of 32 + 2), 4096 (64 rows), D = 1 with M P = 512 (two
   slices), D = 16 with slices of 3 pairs that straddle queries, D = 10, P = 6, M = 25; both triangles from one sum;
F  the model batch, B in {2, 8}, every model with its own operands: each block against the reference and against the bits of
   that model called alone;      G  six calls on one new handle: the shared ticket counters;      H  the refusals.

A fresh handle with the options `gram_log` (every call's GPKSMALL line is asserted against `small_form`) and `debug_fill` (the
serving work area is NaN before every call).  X, alpha and W are views into NaN-filled device buffers with 4 KiB of NaN before
and behind; W holds NaN in its strict upper triangle (vmul and small_wtv_grad_body select 0 there, they do not multiply - read, and
confirmed by every case) and in the pitch columns of ldw = Np + 2.  Host outputs start as NaN with a NaN guard behind them.  Every
case runs twice and must give identical bits; the operands' guards must still be NaN.  e / bar per output is printed per case.

Predicted from reading the code, and found:
* predicted: the index arithmetic of all seven kernels is right and every case passes on the unchanged kernels.  Found: so it is -
  all 52 tests passed at the first run; the library is unchanged but for the GPKSMALL log line;
* predicted: W's strict upper triangle and pitch columns are never multiplied (vmul: `k0 <= row ? a : 0`; small_wtv_grad_body: `r < j`
  -> w = 0; no load reaches column Np).  Found: no NaN in any output;
* predicted: gpk_padded makes Np a multiple of 128, so no call has Np = 576 and nine chunks at most.  Found: Np = 640 holds the nine-chunk
  row blocks (tests/test_small_refs.py);
* predicted: a model's dvar inside a batch cannot have the bits of the model called alone where the row chunks of the W^T V launch
  differ - rc = 256 / (gb B), DESIGN.md and include/gpk.h claim the bits for B = 1 only.  Found: so it is, in all 16 blocks of the two
  batch gradient cases (alone rc 4, batch rc 2 and rc 1): the two differ by at most 2.2e-4 of a bar; mean, var and dmean - and every
  output of the predict, cov and hess batches - have the bits of the model alone.  test_model_batch asserts bit equality for
  those and the sum of the two bars for dvar where rc differs;
* not predicted: the ticket counters cannot be read from outside the library (group G checks them by what the next call returns);
  a share past the last training row is exactly zero, so a dropped last share of the W^T V sum shows only where N reaches the last
  column block (fault 8 below).

Measured on an MI355X, e / bar per group (smallest .. largest over the group's cases; every case prints its own):
* A: mean 4.2e-3 .. 4.7e-2 (N = 33, D = 1, M = 64);   B: mean 9.8e-4 .. 4.2e-2, var 4.7e-6 .. 4.0e-3 (N = 1);
* C: mean 1.3e-3 .. 1.4e-2, cov 4.2e-6 .. 3.3e-3;   D: mean 2.0e-3 .. 1.2e-2, dmean 1.2e-4 .. 1.9e-2, var 3.3e-6 .. 2.0e-4, dvar 5.7e-6 .. 2.4e-4;
* E: mean 5.8e-4 .. 2.9e-2, dmean 8.1e-4 .. 3.1e-2, hess 7.4e-4 .. 3.5e-2 (N = 1);   F: mean .. 1.7e-2, var .. 3.0e-4, cov .. 3.7e-3, dmean
  .. 2.3e-2, dvar .. 2.1e-4, hess .. 2.2e-2.  The bars are worst-case first-order bounds on absolute values: outputs behind W (random signs,
  sums of thousands of terms) use 1e-5 .. 1e-3 of theirs, the others a few hundredths - as plain fp64 NumPy does (at most 0.047).
The same cases against eight deliberately wrong builds of gpk_small.hip (arithmetic or a loop bound only, no address moved), each run
once; tests failed, and the cases over their bar with e / bar:
1  sum_shares stops after its first round: 18 tests - mean where a part adds more than 8 shares (N = 300 .. 4000: 1.4e12 .. 9.6e12), var at 136 shares
   (N = 2100: 1.9e9), every covariance with more than 8 workgroups in a group (Np >= 256: 7.9e9 .. 1.3e12), hess from 12 groups
   (Np = 384: 1.2e13; Np = 2176, 4096: 1.6e12, 2.0e12);
2  small_v_rows without the n2 reload: 7 tests, exactly the cases with 18 or more chunks - var (Np = 1152: 2.1e9, 1.9e9; 2176: 5.8e9),
   cov (Np = 2176: 5.8e9), grad (Np = 2048, 2176: var 7.7e9, 6.8e9, dvar 9.4e8, 6.3e8);
3  finish_means adds 2 of its 4 parts: 32 tests, every case with M P <= 64 and training rows behind the second mean share (mean 8.8e11 .. 3.3e13); none
   of the 2-part and 1-part cases;
4  the covariance's top level drops its last group: 5 tests, every covariance with two or more groups (Np = 384: 2.0e11, 2.1e11, 1.7e11;
   Np = 2176: 1.9e9, 1.4e9);
5  the W^T V span rounded down: 6 tests, every gradient case with rc 4 or 2 (dvar 9.6e7 at Np = 2048 .. 3.1e11 at Np = 128), none at rc 1
   (Np = 2176; B = 8, Np = 512), where Np - j0 is a multiple of 16 and the fault changes nothing;
6  the Hessian's final sum one pair short in slices of several pairs (hess_slice one pair too LONG was not run: two workgroups would
   then carry one entry through the same share - a race, not a wrong bound): 8 tests, every Hessian case of more than one pair (hess
   6.9e12 .. 1.8e16, and entries that must be exactly zero);
7  the Hessian's carry share[t] dropped after round 0: 2 tests, the two-round cases Np = 2176 (32 + 2 rows: 1.7e12) and 4096 (8.8e11);
8  the final W^T V sum drops its last share: 1 test, B = 8, N = Np = 512 (dvar 2.5e9) - elsewhere that share is exactly zero (columns
   past N, or an empty last row chunk).
"""
import ctypes as C
import sys

import numpy as np
import pytest

from test_small_refs import (GROUPS, SEQUENCE, SQ, Case, call_of, case_bars, case_id, case_lines, case_operands, default_hp, form_words,
                             outputs_of, padded, ratio, small_reference)

pytestmark = pytest.mark.gpu

GUARD = 512               # fp64 elements of NaN before and behind every device operand: 4 KiB
HGUARD = 64               # fp64 elements of NaN behind every host output


@pytest.fixture(scope="module")
def be():
    from unmanned_aerial_vehicles_amd.device import Backend
    b = Backend(0).set_options(gram_log=1, debug_fill=1)
    yield b
    b.lib.gpk_destroy(b.h)


def small_lines(capfd):
    """The words of the GPKSMALL lines (option gram_log) written to stderr since the last call."""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    return [ln.split()[1:] for ln in cap.err.splitlines() if ln.startswith("GPKSMALL ")]


def guarded(be, a):
    """(the whole buffer, a view of it holding the fp64 array `a`; NaN entries of `a` stay NaN): NaN before and behind the view."""
    import torch
    buf = torch.full((a.size + 2 * GUARD,), float("nan"), dtype=torch.float64, device=be.device)
    view = buf[GUARD:GUARD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a, dtype=np.float64)))      # (a copy: the cached operands are read-only)
    assert view.data_ptr() == buf.data_ptr() + 8 * GUARD and view.data_ptr() % 16 == 0
    return buf, view


_dev = {}


def dev_case(be, c):
    """The operands of a case on the device, once: per model the guarded views of X, alpha and W (Np x ldw: NaN above the diagonal
    and in the pitch columns)."""
    if c not in _dev:
        ops = case_operands(c)
        Np = padded(c.N)
        d = dict(ops=ops, bufs=[], X=[], alpha=[], W=[])
        for b in range(c.B):
            Wp = np.full((Np, Np + c.pad), np.nan)
            Wp[:, :Np] = np.where(np.tri(Np, dtype=bool), ops["W"][b], np.nan)
            for k, a in (("X", ops["X"][b]), ("alpha", ops["alpha"][b]), ("W", Wp)):
                buf, view = guarded(be, a)
                d["bufs"].append(buf)
                d[k].append(view)
        _dev[c] = d
    return _dev[c]


def _hp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _ptrs(views, models, off=0):
    return np.array([views[b].data_ptr() + off for b in models], dtype=np.uint64)


def shapes(c, B):
    return dict(mean=(B, c.M, c.P), var=(B, c.M), cov=(B, c.M, c.M), dmean=(B, c.M, c.P, c.D), dvar=(B, c.M, c.D), hess=(B, c.M, c.P, c.D, c.D))


def invoke(be, c, d, out, models=None, multi=None, M=None, ldw=None, w_off=0):
    """One call of the case's entry into the host buffers `out` ({output: fp64 array}); models: the models served (all).  Returns the status."""
    ops, lib, h = d["ops"], be.lib, be.h
    models = list(range(c.B)) if models is None else models
    multi = c.entry.startswith("multi_") if multi is None else multi
    B, N, D, P, Np = len(models), c.N, c.D, c.P, padded(c.N)
    M = c.M if M is None else M
    ldw = Np + c.pad if ldw is None else ldw
    outs, call = outputs_of(c), call_of(c)
    factors = "var" in outs or "cov" in outs
    ls = np.ascontiguousarray(np.stack([ops["ls"][b] for b in models]))
    sel = np.concatenate([np.arange(b * P, (b + 1) * P) for b in models])
    ym, ys = np.ascontiguousarray(ops["ym"][sel]), np.ascontiguousarray(ops["ys"][sel])
    sf2, kss, noise = (np.array([ops[k][b] for b in models]) for k in ("sf2", "kss", "noise"))
    Xq = np.ascontiguousarray(ops["Xq"])
    o = {k: _hp(out.get(k)) for k in ("mean", "var", "cov", "dmean", "dvar", "hess")}
    if multi:
        Xp, ap, Wp = _ptrs(d["X"], models), _ptrs(d["alpha"], models), _ptrs(d["W"], models, w_off)
        head = (h, B, _hp(Xp), _hp(ap), N, D, _hp(ls), _hp(sf2), _hp(ym), _hp(ys))
        Wa = _hp(Wp) if factors else None
        if call == "predict":
            return lib.gpk_predict_host_multi(*head, Wa, Np, ldw, _hp(kss) if factors else None, ops["floor"], _hp(Xq), M, o["mean"], o["var"])
        if call == "cov":
            return lib.gpk_predict_host_multi_cov(*head, Wa, Np, ldw, _hp(noise), _hp(Xq), M, o["mean"], o["cov"])
        if call == "grad":
            return lib.gpk_predict_host_multi_grad(*head, Wa, Np, ldw, _hp(kss) if factors else None, ops["floor"], _hp(Xq), M, o["mean"], o["var"],
                                                   o["dmean"], o["dvar"])
        return lib.gpk_predict_host_multi_hess(*head, _hp(Xq), M, o["mean"], o["dmean"], o["hess"])
    b = models[0]
    head = (h, C.c_void_p(d["X"][b].data_ptr()), C.c_void_p(d["alpha"][b].data_ptr()), N, D, P, _hp(ls), float(sf2[0]), _hp(ym), _hp(ys))
    Wa = C.c_void_p(d["W"][b].data_ptr() + w_off) if factors else None
    if call == "predict":
        return lib.gpk_predict_host(*head, Wa, Np, ldw, float(kss[0]), ops["floor"], _hp(Xq), M, o["mean"], o["var"])
    if call == "cov":
        return lib.gpk_predict_host_cov(*head, Wa, Np, ldw, float(noise[0]), _hp(Xq), M, o["mean"], o["cov"])
    if call == "grad":
        return lib.gpk_predict_host_grad(*head, Wa, Np, ldw, float(kss[0]), ops["floor"], _hp(Xq), M, o["mean"], o["var"], o["dmean"], o["dvar"])
    return lib.gpk_predict_host_hess(*head, _hp(Xq), M, o["mean"], o["dmean"], o["hess"])


def nan_outputs(c, B):
    return {k: np.full(int(np.prod(shapes(c, B)[k])) + HGUARD, np.nan) for k in outputs_of(c)}


def run_once(be, capfd, c, models=None, multi=None):
    """One call into NaN host outputs: status 0, the GPKSMALL lines of the mirror, every output written from nothing that is NaN,
    nothing written behind it.  Returns {output: array in the entry's layout}."""
    d = dev_case(be, c)
    B = c.B if models is None else len(models)
    out = nan_outputs(c, B)
    small_lines(capfd)
    be.bind_stream()
    rc = invoke(be, c, d, out, models, multi)
    if rc:                      # a failed launch or a device fault: nothing more is started on the device
        pytest.exit(f"{c.entry} on {case_id(c)}: status {rc}: {be.lib.gpk_last_error(be.h).decode()}", returncode=3)
    want = case_lines(c._replace(B=B))
    lines = small_lines(capfd)
    assert lines == want, (lines, want)
    res = {}
    for k, a in out.items():
        n = a.size - HGUARD
        assert np.isnan(a[n:]).all(), f"nothing behind {k} may be written"
        assert not np.isnan(a[:n]).any(), f"every entry of {k} is written, from nothing that is NaN"
        res[k] = a[:n].reshape(shapes(c, B)[k]).copy()
    return res


_got = {}


def run(be, capfd, c):
    """The case twice with identical bits, the operands' guards still NaN; cached."""
    import torch
    if c not in _got:
        r0, r1 = run_once(be, capfd, c), run_once(be, capfd, c)
        for k in r0:
            assert np.array_equal(r0[k].view(np.int64), r1[k].view(np.int64)), f"{k}: two runs must give identical bits"
        for buf in dev_case(be, c)["bufs"]:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
        _got[c] = r0
    return _got[c]


def check_values(c, got, group, models=None, check=True):
    """Every output within its bar; e / bar printed per output.  models: the blocks of the reference that `got` holds."""
    hp, ref, bars = default_hp(), small_reference(c), case_bars(c)
    sel = slice(None) if models is None else models
    worst = {}
    for k in outputs_of(c):
        entry = (ref[k][0][sel], ref[k][1][sel])
        bar = bars[k][sel]
        r = ratio(hp.f64(np.abs(hp.arr(got[k]) - entry[1])), bar)
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        worst[k] = (float(r[i]), float(np.abs(got[k] - entry[0])[i]), float(bar[i]))
    print(f"{group} {case_id(c)}: " + ", ".join(f"{k} e / bar {w[0]:.1e} (e {w[1]:.2e}, bar {w[2]:.2e})" for k, w in worst.items()))
    if check:
        assert_within(worst)
    return worst


def assert_within(worst):
    for k, w in worst.items():
        assert w[0] <= 1.0, (k, w)


def check_structure(c, got):
    """What holds to the bit whatever the values: the far query, the clip, the symmetries."""
    ops, ref = case_operands(c), small_reference(c)
    M, P = c.M, c.P
    if M >= 5:      # the far query's kernel row is exactly zero
        assert np.array_equal(got["mean"][:, M - 1, :].reshape(-1), ops["ym"][:c.B * P])
        if "var" in got and c.regime != "clip":
            assert np.array_equal(got["var"][:, M - 1], np.array(ops["kss"]))
        for k in ("dmean", "dvar", "hess"):
            if k in got:
                assert not got[k][:, M - 1].any()
    if c.regime == "clip":
        clipped = ref["_raw"] < ops["floor"]
        assert clipped.any() and np.array_equal(got["var"][clipped], np.full(int(clipped.sum()), ops["floor"])) and (got["var"][~clipped] > ops["floor"]).all()
    if "cov" in got:
        cov = got["cov"]
        assert np.array_equal(cov.view(np.int64), np.swapaxes(cov, 1, 2).copy().view(np.int64)), "the covariance is symmetric to the bit"
        if M >= 4:      # queries 2 and 3 are the same row: their cross term carries no noise, their diagonal entries do
            for b in range(c.B):
                noise = ops["noise"][b]
                assert abs((cov[b, 2, 2] - cov[b, 3, 2]) - noise) <= 4 * case_bars(c)["cov"][b, 2, 2] and cov[b, 2, 2] == cov[b, 3, 3]
    if "hess" in got:
        hs = got["hess"]
        assert np.array_equal(hs.view(np.int64), np.swapaxes(hs, 3, 4).copy().view(np.int64)), "both triangles come from one sum"


def check_case(be, capfd, c, group):
    got = run(be, capfd, c)
    worst = check_values(c, got, group, check=False)      # (the figures are printed before anything is asserted)
    check_structure(c, got)
    assert_within(worst)
    return got, worst


# ---- A .. E: one model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUPS["A"], ids=case_id)
def test_mean_only(be, capfd, c):
    check_case(be, capfd, c, "A")
    assert len(case_lines(c)) == (2 if c.M > SQ else 1)


@pytest.mark.parametrize("c", GROUPS["B"], ids=case_id)
def test_mean_and_variance(be, capfd, c):
    check_case(be, capfd, c, "B")


@pytest.mark.parametrize("c", GROUPS["C"], ids=case_id)
def test_covariance(be, capfd, c):
    check_case(be, capfd, c, "C")


@pytest.mark.parametrize("c", GROUPS["D"], ids=case_id)
def test_gradients(be, capfd, c):
    got, _ = check_case(be, capfd, c, "D")
    if c.entry == "grad_var" and c.B == 1:      # the three-launch call's mean and variance are the two-launch call's
        p = run(be, capfd, c._replace(entry="predict_var"))
        assert np.array_equal(p["mean"], got["mean"]) and np.array_equal(p["var"], got["var"])


@pytest.mark.parametrize("c", GROUPS["E"], ids=case_id)
def test_hessian(be, capfd, c):
    got, _ = check_case(be, capfd, c, "E")
    j = run(be, capfd, c._replace(entry="grad"))      # mean and Jacobian come from the gradient call's launch and have its bits
    assert np.array_equal(j["mean"], got["mean"]) and np.array_equal(j["dmean"], got["dmean"])


# ---- F: the model batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUPS["F"], ids=case_id)
def test_model_batch(be, capfd, c):
    got, _ = check_case(be, capfd, c, "F")
    rc_alone, rc_batch = form_words(c._replace(B=1))[10], form_words(c)[10]
    for b in range(c.B):
        alone = run_once(be, capfd, c, models=[b])
        check_values(c, alone, f"F model {b} alone", models=[b])
        for k in outputs_of(c):
            same = np.array_equal(alone[k][0].view(np.int64), got[k][b].view(np.int64))
            if k == "dvar" and rc_alone != rc_batch:
                # gpk_small_launch: rc = 256 / (gb B) row chunks of the W^T V launch, so model b alone adds C = W^T V and the shares
                # of dvar in another order than inside the batch: bit equality cannot hold for this one output (include/gpk.h claims
                # it for B = 1 only); both lie within their bars of the reference, so within the sum of their bars of each other
                bar = case_bars(c)["dvar"][b]
                print(f"F {case_id(c)} model {b}: dvar alone ({rc_alone}) against the batch ({rc_batch}): bits {'equal' if same else 'differ'}, "
                      f"largest difference / bar {float(np.max(ratio(np.abs(alone[k][0] - got[k][b]), bar))):.1e}")
                assert (np.abs(alone[k][0] - got[k][b]) <= 2 * bar).all()
            else:
                assert same, f"model {b}, {k}: the bits of the model called alone"


# ---- G: the shared counters --------------------------------------------------------------------------------------------
def test_sequence_on_one_handle(be, capfd):
    """cov (B = 8) -> hess -> grad (all four) -> cov (B = 1) -> predict twice on one new handle: the covariance's group and top
    tickets, the Hessian's slice tickets and the W^T V ticket share one block of counters, each left at zero by its last workgroup.
    The counters are not readable from outside; a ticket left behind would elect no last workgroup in the next call (NaN outputs)
    or elect it early (other bits), so every result must have the bits of its case's own run."""
    from unmanned_aerial_vehicles_amd.device import Backend
    alone = [run(be, capfd, c) for c in SEQUENCE]
    be2 = Backend(0).set_options(gram_log=1, debug_fill=1)
    try:
        for c, want in zip(SEQUENCE, alone):
            got = run_once(be2, capfd, c)
            for k in outputs_of(c):
                assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), (case_id(c), k)
    finally:
        be2.lib.gpk_destroy(be2.h)


# ---- H: the refusals ---------------------------------------------------------------------------------------------------
def test_refusals(be, capfd):
    from unmanned_aerial_vehicles_amd import _lib
    Np = 128
    calls = []
    for entry in ("predict_var", "cov", "grad_var"):
        c1, c8 = Case("H", entry, 100, 9, 1, 5, 1, 2, "plain"), Case("H", "multi_" + entry, 100, 9, 1, 5, 2, 2, "plain")
        for c in (c1, c8):
            calls += [(c, "W off by 8 bytes", dict(w_off=8)), (c, "odd ldw", dict(ldw=Np + 1)), (c, "ldw < Np", dict(ldw=Np - 2)),
                      (c, "M = 0", dict(M=0))]
        calls.append((c8, "M = 33 on a multi entry", dict(M=33)))
    ch = Case("H", "multi_hess", 100, 9, 1, 5, 2, 0, "plain")
    calls += [(ch, "M = 0", dict(M=0)), (ch, "M = 33 on a multi entry", dict(M=33)), (Case("H", "hess", 100, 9, 1, 5, 1, 0, "plain"), "M = 0", dict(M=0))]
    for c, what, kw in calls:
        d = dev_case(be, c)
        out = nan_outputs(c._replace(M=max(c.M, kw.get("M", 0))), c.B)
        small_lines(capfd)
        be.bind_stream()
        rc = invoke(be, c, d, out, **kw)
        msg = be.lib.gpk_last_error(be.h).decode()
        assert rc == _lib.GPK_BAD_ARG and msg.startswith("bad argument"), (c.entry, what, rc, msg)
        be.sync()
        assert small_lines(capfd) == [], "a refused call must not launch"
        assert all(np.isnan(a).all() for a in out.values()), (c.entry, what)
    # ... and the same arguments are accepted once nothing is wrong with them
    for c in dict.fromkeys(c for c, _, _ in calls):
        check_values(c, run(be, capfd, c), "H")
