"""Every launch form of the matrix-core posterior mean (gpk_predict_mean_mfma, gpk_mean.hip: mean_prep_kernel, mean_bf16_kernel for
D <= 14, mean_mfma_kernel<9> for D = 15, 16, mean_mfma_reduce_kernel) called directly through the C ABI on operands the test builds
itself - no fitted model - against the fp64 reference, the launch-rule mirror and the bars of tests/test_mean_mfma_refs.py:

A  bf16, every instantiation: P = 1 .. 8 at D = 9, N = 200, M = 300 (the last workgroup partly and wholly past M in both layouts);
B  bf16, where the `1` and |u_q|^2 components sit: D in {1, 6, 7, 8, 13, 14} x P in {3, 5};
C  bf16, the pipeline and the chunks: one block, an odd and an even count, the ragged last block (1, 4, 8, 20 points), two to five
   chunks, 64 blocks in one workgroup (S = 1), 48 + 48 + 33 blocks, M = 1, 255, 256, 257 - for P = 3 (QB 2) and P = 4 (QB 1);
D  fp32-MFMA: D = 15, 16 x P = 1 .. 8; N = 1, 33, 513; two staging rounds in one workgroup; rounds of 512, 512 and 4;
E  the gate regime, 48 <= |u|^2 <= 64 by the `center` argument alone, and the same data centred: the two within the sum of their bars;
F  alpha with random signs, and queries that are training rows;      G  the reduce step;      H  the refusals.

A fresh handle with the options `gram_log` (every case asserts the library's own GPKMEANMM line against `mean_mfma_form`) and
`debug_fill` (the partial sums in the handle's scratch start as NaN at every call).  X, alpha and Xq are views into NaN-filled
device buffers with 4 KiB of NaN before and behind; the output starts as NaN and keeps a NaN guard behind row M.  Every case runs
twice and must give identical bits.  e = the largest |mean_gpu - mean| over queries and outputs relative to y_std sf2 s (regimes
"share", "gate") or y_std sf2 sqrt(sum_j (k_mj alpha_jp)^2) ("signed"), against bar = 4 e_full of the case's complete emulation
(and a quarter of the error of a claimed second-order product), from the reference side alone.

Predicted from reading the code, and found:
* predicted: the index arithmetic of all four kernels is right and every case passes on the unchanged kernels.  Found: so it is -
  every case passed at the first run; the library is unchanged but for the log line.  The emulation turned out to be close to the
  kernels bit for bit: in 39 of the 88 runs e equals the emulation's error to three digits;
* predicted: a missing second-order product shows at the gate and not centred.  Found: only a2 b0 does (34 .. 51 e_full, claimed by
  every bf16 gate case); a0 b2 and a1 b1 average out over the training points (1.5 .. 1.9 e_full) and no case claims them
  (tests/test_mean_mfma_refs.py);
* not predicted: standard normal rows cannot all lie in 48 <= |u|^2 <= 64 whatever the centre (the gate cases contract them by 1 / 4),
  and a ragged last block cannot hold a share floor for every query (asked of the whole blocks; dropping it is a planted fault).

Measured on an MI355X, per group (e / the complete emulation's error / bar; every case prints its own):
* A: e 4.3e-7 .. 5.2e-7 against bars 1.7e-6 .. 2.1e-6;   B: 3.2e-7 .. 9.4e-7 (D = 1, P = 5: 9.4e-7 / 6.6e-7 / 2.7e-6);
* C: 8.2e-8 (M = 1) .. 1.4e-5 (N = 1, whose exponents reach 25: 1.4e-5 / 1.4e-5 / 5.5e-5); closest to its bar N = 2048, M = 262 149:
  8.7e-7 / 3.8e-7 / 1.5e-6 - the emulation sees 384 of those queries, the launch all of them; N = 4100, M = 90 000: 6.9e-7 / 4.1e-7 / 1.7e-6;
* D: 2.7e-7 .. 9.8e-7 (N = 1); N = 1024, M = 262 144: 6.0e-7 / 4.0e-7 / 1.6e-6; N = 4100: 6.0e-7 / 3.9e-7 / 1.5e-6;
* E: at the gate 5.8e-6 .. 6.8e-6 / 5.6e-6 .. 6.7e-6 / 2.2e-5 .. 2.7e-5, centred 2.1e-7 .. 2.5e-7 / 1.9e-7 .. 2.4e-7 / 7.6e-7 .. 9.5e-7, the two
  runs 5.8e-6 .. 6.9e-6 apart;   F: 6.1e-7 / 6.1e-7 / 2.5e-6, 6.1e-7 / 5.2e-7 / 2.1e-6, queries on training rows 8.3e-7 / 5.7e-7 / 2.3e-6;
* G: bf16, 5 chunks: identical to the epilogue of the fp64 sum of the per-chunk calls; fp32-MFMA, 6 chunks: 2 ulp of the largest term
  (1 ulp of a result one binade above it).  No case uses more than 0.56 of its bar.
The same cases against five deliberately wrong builds of gpk_mean.hip (arithmetic only, no address moved); cases over their bar, e:
1  chain6 without a1 b0: all 57 bf16 cases (groups A, B, C, F, G 2.8e-3 .. 2.6e-2, gate 0.18 .. 0.22), 390 to 10 000 bars;
2  chain6 without a0 b2: 10 cases, none of them at the gate, where no case claims it - D = 1 (1.5e-5 and 1.6e-5, 6 bars), the signed
   cases (8.3e-6 and 9.2e-6, 3.4 and 4.0 bars), and by 1.0 to 1.6 bars D = 6 P = 5 and N = 20, 32, 33;
3  the block loop of mean_bf16_kernel one block short: all 57 bf16 cases, 2.6e-2 .. 1.0 (N <= 32: nothing is left);
4  the mask-1 exchange of QB = 1 left out: 28 of the 29 bf16 cases with P >= 4 (0.50 .. 0.72, signed 1.7), all but N = 1, whose only
   point sits in lane 0 and whose partner holds zero;
5  nblk of mean_mfma_kernel rounded down: 24 of the 25 fp32-MFMA cases (3.3e-3 .. 1.0), all but N = 1024 (whole blocks only).
"""
import ctypes as C
import sys

import numpy as np
import pytest

from test_mean_mfma_refs import (GATE0, GROUPS, SF2, Case, case_figures, case_id, case_operands, form_words, mean_mfma_form, mean_reference,
                                 reduce_epilogue)

pytestmark = pytest.mark.gpu

GUARD = 1024              # fp32 elements of NaN before and behind every operand: 4 KiB
PANEL = 8192              # queries per panel of the reference on the device


@pytest.fixture(scope="module")
def be():
    from unmanned_aerial_vehicles_amd.device import Backend
    b = Backend(0).set_options(gram_log=1, debug_fill=1)
    yield b
    b.lib.gpk_destroy(b.h)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dp(a):
    from unmanned_aerial_vehicles_amd import _lib
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_lib._dp) if a is not None else None


def mm_lines(capfd):
    """The words of the GPKMEANMM lines (option gram_log) written to stderr since the last call."""
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    return [ln.split()[1:] for ln in cap.err.splitlines() if ln.startswith("GPKMEANMM ")]


def guarded(be, a):
    """(the whole buffer, a view of it holding the fp32 array `a`): NaN in the GUARD elements before and behind the view."""
    import torch
    buf = torch.full((a.size + 2 * GUARD,), float("nan"), dtype=torch.float32, device=be.device)
    view = buf[GUARD:GUARD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    assert view.data_ptr() == buf.data_ptr() + 4 * GUARD
    return buf, view


_dev = {}


def dev_case(be, c):
    """The operands of a case on the device, once: the guarded views and the NumPy operands."""
    if c not in _dev:
        ops = case_operands(c)
        d = dict(ops=ops)
        for k in ("X", "alpha", "Xq"):
            d[k + "_buf"], d[k] = guarded(be, ops[k])
        _dev[c] = d
    return _dev[c]


def call(be, d, c, out, *, X=None, alpha=None, N=None, sf2=SF2, ym=None, ys=None):
    ops = d["ops"]
    return be.lib.gpk_predict_mean_mfma(be.h, _p(d["X"] if X is None else X), _p(d["alpha"] if alpha is None else alpha), c.N if N is None else N,
                                        c.D, c.P, _dp(ops["ls"]), sf2, _dp(ops["center"]), _dp(ops["ym"] if ym is None else ym),
                                        _dp(ops["ys"] if ys is None else ys), _p(d["Xq"]), c.M, _p(out))


def run(be, capfd, c, **kw):
    """gpk_predict_mean_mfma twice into NaN outputs with a NaN guard behind row M; the GPKMEANMM line of each call asserted against
    the mirror; the operands' guards still NaN.  Returns the (M, P) fp32 result on the device."""
    import torch
    d = dev_case(be, c)
    want = form_words(kw.get("N", c.N), c.M, c.D, c.P)
    outs = []
    for _ in range(2):
        out = torch.full((c.M * c.P + GUARD,), float("nan"), dtype=torch.float32, device=be.device)
        mm_lines(capfd)
        be.bind_stream()
        for rc in (call(be, d, c, out, **kw), be.lib.gpk_synchronize(be.h)):
            if rc:                      # a failed launch or a device fault: nothing more is started on the device
                pytest.exit(f"gpk_predict_mean_mfma on {case_id(c)}: status {rc}: {be.lib.gpk_last_error(be.h).decode()}", returncode=3)
        lines = mm_lines(capfd)
        assert lines == [want], (lines, want)
        assert bool(torch.isnan(out[c.M * c.P:]).all()), "nothing behind row M may be written"
        assert not bool(torch.isnan(out[:c.M * c.P]).any()), "every output is written, from nothing that is NaN"
        outs.append(out[:c.M * c.P].view(c.M, c.P))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs must give identical bits"
    for k in ("X", "alpha", "Xq"):
        buf = d[k + "_buf"]
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
    return outs[0]


def reference(be, c):
    """(mean, den) fp64 torch tensors (M, P) of a case, once: on the CPU, or in panels on the device for more than 2048 queries."""
    import torch
    d = dev_case(be, c)
    if "ref" not in d:
        ops, signed = d["ops"], c.regime.startswith("signed")
        if c.M <= 2048:
            d["ref"] = mean_reference(ops, ops["Xq"], signed)
        else:
            parts = [mean_reference(ops, d["Xq"][m0:m0 + PANEL].double(), signed, device=be.device) for m0 in range(0, c.M, PANEL)]
            d["ref"] = (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
    return d["ref"]


def gpu_err(be, c, got):
    mean, den = reference(be, c)
    return float(((got.double().to(mean.device) - mean).abs() / den).max())


def check_case(be, capfd, c, group):
    g = case_figures(c)
    got = run(be, capfd, c)
    e = gpu_err(be, c, got)
    f = g["form"]
    print(f"{group} {case_id(c)}: {f.kernel} qb{f.QB} nqb{f.nqb} s{f.S} chunk{f.chunk} nb{list(f.nb)} last{f.last}: "
          f"e {e:.2e}, emulation {g['e_full']:.2e}, claims {list(g['claims'])}, bar {g['bar']:.2e}")
    assert e <= g["bar"], (e, g["bar"])
    return got, g


# ---- A .. D, F: one call per case -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUPS["A"], ids=case_id)
def test_bf16_every_instantiation(be, capfd, c):
    _, g = check_case(be, capfd, c, "A")
    assert g["form"].kernel == "bf16" and g["form"].QB == (2 if c.P <= 3 else 1) and g["form"].nqb == (2 if c.P <= 3 else 3)


@pytest.mark.parametrize("c", GROUPS["B"], ids=case_id)
def test_bf16_component_positions(be, capfd, c):
    _, g = check_case(be, capfd, c, "B")
    assert g["form"].kernel == "bf16"


@pytest.mark.parametrize("c", GROUPS["C"], ids=case_id)
def test_bf16_pipeline_and_chunk_edges(be, capfd, c):
    _, g = check_case(be, capfd, c, "C")
    f = g["form"]
    assert f.kernel == "bf16"
    if c.N == 2048:
        assert (f.S, f.nb) == (1, (64,))
    if c.N == 4100:
        assert (f.S, f.nb, f.last) == (3, (48, 48, 33), 4)


@pytest.mark.parametrize("c", GROUPS["D"], ids=case_id)
def test_f32_mfma_forms(be, capfd, c):
    _, g = check_case(be, capfd, c, "D")
    f = g["form"]
    assert f.kernel == "f32"
    if c.N == 1024:
        assert f.rounds == ((512, 512),)
    if c.N == 4100:
        assert f.rounds[-1] == (512, 512, 4)


@pytest.mark.parametrize("c", GROUPS["F"], ids=case_id)
def test_signed_alpha(be, capfd, c):
    check_case(be, capfd, c, "F")


# ---- E: the gate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUPS["E"], ids=case_id)
def test_gate_regime(be, capfd, c):
    c0 = GATE0[GROUPS["E"].index(c)]
    got, g = check_case(be, capfd, c, "E")
    got0, g0 = check_case(be, capfd, c0, "E")
    assert np.array_equal(case_operands(c)["X"], case_operands(c0)["X"]) and not np.array_equal(case_operands(c)["center"], case_operands(c0)["center"])
    den = reference(be, c)[1]
    diff = float(((got.double().cpu() - got0.double().cpu()).abs() / den).max())
    print(f"E {case_id(c)}: off-centre against centred {diff:.2e}, bars {g['bar']:.2e} + {g0['bar']:.2e}")
    assert diff <= g["bar"] + g0["bar"]


# ---- G: the reduce step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GROUPS["G"], ids=case_id)
def test_reduce_step(be, capfd, c):
    """The partial sums of every chunk, from one call per chunk (S = 1, sf2 = 1, y_mean = 0, y_std = 1: the output IS the partial
    sum), added in fp64 and put through the epilogue: the whole call's result within 2 ulp of the largest term."""
    got, g = check_case(be, capfd, c, "G")
    f = g["form"]
    assert f.S >= 5 and f.chunk == 512
    d = dev_case(be, c)
    total = np.zeros((c.M, c.P))
    for s in range(f.S):
        n0, n1 = s * f.chunk, min(c.N, (s + 1) * f.chunk)
        part = run(be, capfd, c, X=d["X"][n0:n1], alpha=d["alpha"][n0:n1], N=n1 - n0, sf2=1.0, ym=np.zeros(c.P), ys=np.ones(c.P))
        assert mean_mfma_form(n1 - n0, c.M, c.D, c.P).S == 1
        total += part.double().cpu().numpy()
    ops = d["ops"]
    want = reduce_epilogue(total, ops)
    term = np.maximum(np.abs(ops["ym"].astype(np.float32)), np.abs(ops["ys"].astype(np.float32) * (np.float32(SF2) * total.astype(np.float32))))
    ulps = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)) / np.spacing(term.astype(np.float32)).astype(np.float64)))
    print(f"G {case_id(c)}: {f.S} chunks: the call against the epilogue of the fp64 chunk sum: {ulps:.2f} ulp of the largest term")
    assert ulps <= 2.0


# ---- H: the refusals --------------------------------------------------------------------------------------------------
def test_refusals(be, capfd):
    import torch
    from unmanned_aerial_vehicles_amd import _lib
    c = Case("share", 200, 300, 9, 3)
    d = dev_case(be, c)
    ops = d["ops"]
    out = torch.full((c.M * 9 + GUARD,), float("nan"), dtype=torch.float32, device=be.device)
    X17 = torch.zeros((c.N, 17), dtype=torch.float32, device=be.device)
    alpha9 = torch.zeros((c.N, 9), dtype=torch.float32, device=be.device)
    ls17, nine = np.ones(17), np.ones(9)

    def f(X=d["X"], alpha=d["alpha"], N=c.N, D=c.D, P=c.P, ls=ops["ls"], center=ops["center"], ym=ops["ym"], ys=ops["ys"], Xq=d["Xq"], M=c.M, mean=out):
        return be.lib.gpk_predict_mean_mfma(be.h, _p(X), _p(alpha), N, D, P, _dp(ls), SF2, _dp(center), _dp(ym), _dp(ys), _p(Xq), M, _p(mean))

    ls0, lsneg = ops["ls"].copy(), ops["ls"].copy()
    ls0[4], lsneg[8] = 0.0, -1.0
    calls = {
        "D = 0": lambda: f(D=0), "D = 17": lambda: f(X=X17, D=17, ls=ls17, center=ls17), "P = 0": lambda: f(P=0),
        "P = 9": lambda: f(alpha=alpha9, P=9, ym=nine, ys=nine), "N = 0": lambda: f(N=0), "M = 0": lambda: f(M=0),
        "N < 0": lambda: f(N=-1), "M < 0": lambda: f(M=-1), "ls = 0": lambda: f(ls=ls0), "ls < 0": lambda: f(ls=lsneg),
        "null X": lambda: f(X=None), "null alpha": lambda: f(alpha=None), "null ls": lambda: f(ls=None), "null center": lambda: f(center=None),
        "null y_mean": lambda: f(ym=None), "null y_std": lambda: f(ys=None), "null Xq": lambda: f(Xq=None), "null mean": lambda: f(mean=None),
    }
    mm_lines(capfd)
    be.bind_stream()
    for what, fn in calls.items():
        rc = fn()
        msg = be.lib.gpk_last_error(be.h).decode()
        assert rc == _lib.GPK_BAD_ARG and msg.startswith("bad argument") and "predict_mean_mfma" in msg, (what, rc, msg)
    be.sync()
    assert mm_lines(capfd) == [], "a refused call must not launch"
    assert bool(torch.isnan(out).all())
    # ... and the same arguments are accepted once nothing is wrong with them
    be.check(f())
    be.sync()
    assert mm_lines(capfd) == [form_words(c.N, c.M, c.D, c.P)] and not bool(torch.isnan(out[:c.M * c.P]).any()) and bool(torch.isnan(out[c.M * c.P:]).all())
