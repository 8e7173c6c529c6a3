"""Host side of tests/test_gpu_deriv_forms.py: the cases, their operands, an extended-precision reference, the mirror of the five
launch rules and the bars of the large-batch derivative kernels (K8: gpk_jac.hip, gpk_hess.hip) - nothing here needs a GPU.

Entries: grad = gpk_predict_mean_grad, grad_multi = gpk_predict_mean_grad_multi, vargrad = gpk_predict_var_grad_inv, hess =
gpk_predict_mean_hess, hess_multi = gpk_predict_mean_hess_multi.  A case's `P` is P (outputs of one model) or B (single-output
models on shared inputs).

Operands (`case_operands`, the layout of test_small_refs.case_operands), from a seed derived from the case:
* X standard normal (shared by the models of a multi call); length-scales per model and feature in [0.7, 2.5] sqrt(D), every model
  its own; alpha: random signs, magnitude in [0.5, 1.5]; sf2 and y_std distinct per output or model;
* queries: standard normal; query 0 is training row 0 and query 1 training row N - 1 (M >= 2), queries 2 and 3 are the same row
  (M >= 4), and the last query of the first period (M >= 5) lies more than 60 length-scales from every training row: its kernel
  row is exactly 0 in fp64 and every derivative there is exactly 0.  A case with M > PERIOD (768 = three workgroups of 256 queries;
  vargrad: 384 = three workgroups of 128 query columns, because its reference costs two Np x N x period long-double products)
  repeats its first period: query m is query m mod period, so that only one period needs a reference;
* vargrad: W a dense random lower-triangular matrix, entries N(0, 1) / sqrt(Np), diagonal positive, as in test_small_refs - but
  rows N .. Np - 1 are zero left of column N, as in every inverse factor of a matrix padded with the identity:
  var_grad_kernel adds the first N rows of V = W K* only (read from its loop bounds - the small-batch kernels add all Np), so the
  literal formula kss - |W k*|^2 holds on such factors alone.  `w_device_image`: the Np x ldw array the device gets - exactly zero
  above the diagonal inside the band of GPK_ZERO_BAND_TILES tiles that gpk_trtri zeroes, NaN beyond it and in the pitch columns.
  Regime "clip": kss lies between the subtracted terms of the queries.

Reference (`deriv_reference`): test_small_refs._model_reference - the formulas of include/gpk.h, literally, in that module's
extended format (HP), differences formed before any product - with its scale and escale per output, exactly as defined there.

Mirror (`deriv_form`): the launch rules of the five entries restated from the C code: per query panel d4, ps | bs, the groups, the
row blocks [R0, R1) of the Hessian's triangle with the rows below D, gran, S, chunk, the staging rounds of the longest chunk and
the rows of the very last round, the Hessian's panel and capS, and the chain of rounding operations behind each output:
  grad        4 (e alpha, x / ls, q / ls -, fma) + rows of the longest chunk + S + 3 (y_std sf2, / ls, *)
  grad_multi  3 (e alpha, x - q, fma) + rows + S + 4 (y_std sf2, l l, /, *)
  hess        7 (e alpha, two differences of two quotients, w df, fma) + rows + S + 1 (- S_p) + 4 (y_std sf2, ls ls, /, *)
  hess_multi  4 (e alpha, raw differences, their product, fma) + rows + S + 4 (1 / l twice, g, s g) + 1 (- S) + 3 (c, c g, *)
  vargrad     V: 1 + Np (K*, then a GEMM of k-length up to Np, an fp64 MFMA counted as four chained FMAs); C: V + Np;
              var = 2 V + 1 + rows + S + 1;  dvar = C + 1 (K* C) + 3 + rows + S + 2 (-2 / ls, *)
Bars: bar = 2^-53 (chain scale + escale), first order; nothing in a bar is taken from a GPU result.

Host tests: the mirror at hand-counted switch points; every switch point is a case; plain fp64 NumPy in three summation orders
within every bar - largest error / bar over all cases and outputs: 0.140 (A-grad-N1-D1-P1-M1: one training row, a chain of 9;
test_small_refs measured 0.047 for its family); one block of 32 training rows, one whole chunk or the last slot of a group removed
moves some entry of every output, and the median query, by at least 100 bars (measured: at least 2.6e6 and 6.9e5, both for the
variance at Np = 2304); the sliced long-double product (`sliced_matmul`, which makes the Np = 2304 reference affordable) is the
plain one, and only the three largest variance-gradient
references take it; the mpmath path agrees with the long-double path on a small case.
"""
import math
import zlib
from collections import namedtuple

import numpy as np
import pytest

import test_small_refs as SR
from test_small_refs import EXP_ULPS, HP, U, default_hp, padded, ratio

Case = namedtuple("Case", "group entry N D P M pad var regime off")
Panel = namedtuple("Panel", "m0 mc d4 gs groups blocks nq gran S chunk rounds tail panel capS chain")

PERIOD = 768
ZERO_BAND_TILES, TILE = 16, 128
MG_PANEL = HS_PANEL = 65536
HS_PARTIAL_BYTES = 256 << 20
JG_TJ = HS_TJ = 128
VG_TJ, VG_COLS = 64, 128
ENTRY_NAME = {"grad": "mean_grad", "grad_multi": "mean_grad_multi", "vargrad": "var_grad", "hess": "mean_hess", "hess_multi": "mean_hess_multi"}
# entry -> (the entry of test_small_refs whose outputs hold ours, our outputs)
_SR = {"grad": ("grad", ("dmean",)), "grad_multi": ("multi_grad", ("dmean",)), "vargrad": ("grad_var", ("var", "dvar")),
       "hess": ("hess", ("hess",)), "hess_multi": ("multi_hess", ("hess",))}


def _c(group, entry, N, D, P, M, pad=0, var=1, regime="plain", off=0):
    return Case(group, entry, N, D, P, M, pad, var, regime, off)


def is_multi(c):
    return c.entry.endswith("_multi")


def period(c):
    return PERIOD // 2 if c.entry == "vargrad" else PERIOD


def ref_m(c):
    """The queries that have a reference: the first period."""
    return min(c.M, period(c))


def outputs_of(c):
    outs = _SR[c.entry][1]
    return tuple(k for k in outs if k != "var" or c.var)


GROUPS = {
    # gpk_predict_mean_grad: the 16 (d4, ps) pairs; P = 5 (3 + 2), 7 (4 + 3), 9 (3 x 3), 13 (4, 4, 4, 1), 16; N and M at every edge;
    # N = 16384 | 16385 at M = 1; chunks of two 128-row rounds, the last one ragged (M = 20000); two panels (M = 65537)
    "A": [_c("A", "grad", 1, 1, 1, 1), _c("A", "grad", 31, 4, 2, 255), _c("A", "grad", 32, 1, 3, 256), _c("A", "grad", 33, 4, 4, 257, off=1),
          _c("A", "grad", 127, 5, 1, 512), _c("A", "grad", 128, 8, 2, 513), _c("A", "grad", 129, 5, 5, 257), _c("A", "grad", 300, 8, 7, 512),
          _c("A", "grad", 300, 9, 1, 513), _c("A", "grad", 129, 12, 2, 1), _c("A", "grad", 33, 9, 9, 255, off=1), _c("A", "grad", 128, 12, 13, 256),
          _c("A", "grad", 127, 13, 1, 257), _c("A", "grad", 300, 16, 2, 512), _c("A", "grad", 31, 13, 3, 513), _c("A", "grad", 300, 16, 16, 257, off=1),
          _c("A", "grad", 16384, 1, 1, 1), _c("A", "grad", 16385, 1, 1, 1), _c("A", "grad", 1000, 1, 16, 20000), _c("A", "grad", 300, 1, 1, 65537)],
    # gpk_predict_mean_grad_multi: the 16 (d4, bs) pairs, B = 1 .. 8 with 5 (3 + 2) and 7 (4 + 3); two panels
    "B": [_c("B", "grad_multi", 1, 1, 1, 1), _c("B", "grad_multi", 33, 4, 2, 256), _c("B", "grad_multi", 128, 1, 3, 257, off=1),
          _c("B", "grad_multi", 129, 4, 4, 513), _c("B", "grad_multi", 300, 5, 1, 512), _c("B", "grad_multi", 31, 8, 2, 255),
          _c("B", "grad_multi", 127, 5, 5, 257), _c("B", "grad_multi", 32, 8, 7, 513, off=1), _c("B", "grad_multi", 300, 9, 1, 1),
          _c("B", "grad_multi", 129, 12, 2, 257), _c("B", "grad_multi", 33, 9, 6, 512), _c("B", "grad_multi", 128, 12, 8, 256),
          _c("B", "grad_multi", 127, 13, 1, 513), _c("B", "grad_multi", 300, 16, 2, 255), _c("B", "grad_multi", 129, 13, 3, 257),
          _c("B", "grad_multi", 33, 16, 4, 512), _c("B", "grad_multi", 33, 1, 5, 65537)],
    # gpk_predict_var_grad_inv: d4 = 1 .. 4; Np in {128, 256, 640} with N = Np and N = Np - 127; M in {1, 127, 128, 129, 300}; ldw = Np and
    # Np + 2; var NULL (var = 0) and not; the clip; Np = 2304: W NaN beyond its zero band; chunks of two 64-row rounds (N M = 1.9e7)
    "C": [_c("C", "vargrad", 128, 1, 1, 1), _c("C", "vargrad", 1, 4, 1, 127, pad=2), _c("C", "vargrad", 256, 5, 1, 128, var=0),
          _c("C", "vargrad", 129, 9, 1, 129, pad=2), _c("C", "vargrad", 640, 13, 1, 300), _c("C", "vargrad", 513, 16, 1, 129, pad=2, var=0),
          _c("C", "vargrad", 300, 9, 1, 128, regime="clip"), _c("C", "vargrad", 2304, 9, 1, 129), _c("C", "vargrad", 640, 4, 1, 29057)],
    # gpk_predict_mean_hess: the seven forms; D = 9: row block [8, 12) holds row 8 alone, D = 13: [13, 16) is empty, D = 14: one row;
    # capS-bound: one chunk of three rounds (M = 8192); the reduced panel of 15104 queries (M = 15105)
    "D": [_c("D", "hess", 1, 1, 1, 1), _c("D", "hess", 33, 2, 2, 256), _c("D", "hess", 129, 3, 3, 257, off=1), _c("D", "hess", 300, 4, 4, 513),
          _c("D", "hess", 33, 4, 5, 257), _c("D", "hess", 129, 3, 7, 256), _c("D", "hess", 300, 2, 16, 257), _c("D", "hess", 33, 5, 1, 513),
          _c("D", "hess", 129, 8, 3, 256), _c("D", "hess", 300, 9, 1, 257, off=1), _c("D", "hess", 33, 12, 3, 1), _c("D", "hess", 129, 13, 1, 256),
          _c("D", "hess", 300, 14, 3, 257), _c("D", "hess", 129, 16, 16, 257, off=1), _c("D", "hess", 300, 16, 16, 8192),
          _c("D", "hess", 33, 16, 16, 15105)],
    # gpk_predict_mean_hess_multi: the seven forms; B = 1 .. 8, odd B above D = 4 (the masked second model of a group); D = 5: [5, 8) is
    # empty, D = 13: [12, 14) holds row 12 alone and [14, 16) is empty, D = 15: one row; two panels at the reduced panel of 48896
    "E": [_c("E", "hess_multi", 1, 1, 1, 1), _c("E", "hess_multi", 33, 4, 2, 256), _c("E", "hess_multi", 129, 1, 3, 257, off=1),
          _c("E", "hess_multi", 300, 4, 4, 513), _c("E", "hess_multi", 33, 4, 5, 257), _c("E", "hess_multi", 129, 1, 7, 256),
          _c("E", "hess_multi", 300, 4, 8, 1), _c("E", "hess_multi", 33, 5, 3, 257), _c("E", "hess_multi", 129, 8, 6, 256),
          _c("E", "hess_multi", 300, 9, 1, 257, off=1), _c("E", "hess_multi", 33, 12, 5, 513), _c("E", "hess_multi", 129, 13, 7, 257),
          _c("E", "hess_multi", 300, 15, 2, 256), _c("E", "hess_multi", 129, 16, 8, 257), _c("E", "hess_multi", 33, 16, 5, 48897)],
}
ALL_CASES = [c for g in GROUPS.values() for c in g]
# group F: six calls of different entries in a row on one handle (the scratch grows, shrinks in use and is refilled with NaN)
SEQUENCE = [GROUPS["D"][13], GROUPS["A"][0], GROUPS["C"][4], GROUPS["E"][11], GROUPS["B"][6], GROUPS["A"][15]]


def case_id(c):
    return f"{c.group}-{c.entry}-N{c.N}-D{c.D}-{'B' if is_multi(c) else 'P'}{c.P}-M{c.M}" + (f"-ldw+{c.pad}" if c.pad else "") + \
        ("" if c.var else "-novar") + ("" if c.regime == "plain" else "-" + c.regime) + ("-off8" if c.off else "")


# ---- the launch rules of the five entries, restated ----------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def tri(d):
    return d * (d + 1) // 2


def _chunking(N, gran, S, capS=None):
    maxS = _ceil(N, gran)
    if capS is not None and S > capS:
        S = capS
    S = min(S, maxS)
    S = max(S, 1)
    S = min(S, 65535)
    chunk = _ceil(_ceil(N, S), gran) * gran
    return _ceil(N, chunk), chunk


def _even_groups(P, most):
    """(number of groups, slots per group): the fewest groups of at most `most`, evenly filled."""
    n = _ceil(P, most)
    return n, _ceil(P, n)


def hess_blocks(entry, d4):
    if entry == "hess":
        return {1: [(0, 4)], 2: [(0, 8)], 3: [(0, 8), (8, 12)], 4: [(0, 9), (9, 13), (13, 16)]}[d4]
    return {1: [(0, 4)], 2: [(0, 5), (5, 8)], 3: [(0, 7), (7, 10), (10, 12)], 4: [(0, 7), (7, 10), (10, 12), (12, 14), (14, 16)]}[d4]


def deriv_form(entry, N, D, PB, M):
    """The launch pairs of one call, a Panel per query panel: gs = ps | bs; groups: (first slot, live slots) per output or model
    group; blocks: (R0, R1, rows below D) per row block; nq: query blocks; rounds: the staging rounds of the longest chunk; tail: the
    rows of the last round of the last chunk; chain: {output: rounding operations}."""
    assert entry in ENTRY_NAME and N >= 1 and M >= 1 and 1 <= D <= 16 and 1 <= PB <= (8 if entry.endswith("_multi") else 16)
    d4 = _ceil(D, 4)
    TP = tri(D) + 1
    panel, blocks = MG_PANEL, [(0, 4 * d4, D)]
    if entry == "vargrad":
        ng, gs, panel = 1, 1, M
    elif entry in ("grad", "grad_multi"):
        ng, gs = _even_groups(PB, 4)
    else:
        if d4 == 1:
            ng, gs = _even_groups(PB, 4)
        elif entry == "hess":
            ng, gs = PB, 1
        else:
            ng, gs = _ceil(PB, 2), 2
        blocks = [(r0, r1, max(0, min(r1, D) - r0)) for r0, r1 in hess_blocks(entry, d4)]
        panel = max(256, min(HS_PANEL, HS_PARTIAL_BYTES // (PB * TP * 8) // 256 * 256))
    groups = [(g * gs, min(gs, PB - g * gs)) for g in range(ng)]
    nz = ng * len(blocks)
    out = []
    for m0 in range(0, M, panel):
        mc = min(panel, M - m0)
        capS = None
        if entry == "vargrad":
            nq, gran, tj = _ceil(mc, VG_COLS), VG_TJ, VG_TJ
        else:
            nq, gran, tj = _ceil(mc, 256), (32 if mc <= 512 and N <= 16384 else 128), 128
            if entry in ("hess", "hess_multi"):
                capS = HS_PARTIAL_BYTES // (mc * PB * TP * 8)
        S, chunk = _chunking(N, gran, _ceil(2048, nq * nz), capS)
        rows = min(chunk, N)
        last = N - (S - 1) * chunk
        tail = last - (_ceil(last, tj) - 1) * tj
        if entry == "grad":
            chain = dict(dmean=4 + rows + S + 3)
        elif entry == "grad_multi":
            chain = dict(dmean=3 + rows + S + 4)
        elif entry == "hess":
            chain = dict(hess=7 + rows + S + 1 + 4)
        elif entry == "hess_multi":
            chain = dict(hess=4 + rows + S + 4 + 1 + 3)
        else:
            v = 1 + padded(N)
            chain = dict(var=2 * v + 1 + rows + S + 1, dvar=(v + padded(N)) + 1 + 3 + rows + S + 2)
        out.append(Panel(m0, mc, d4, gs, groups, blocks, nq, gran, S, chunk, _ceil(rows, tj), tail, panel, capS, chain))
    return out


def form_words(entry, N, D, PB, pn):
    """The words of the library's GPKDERIV line (option gram_log) for one launch pair."""
    multi, var = entry.endswith("_multi"), entry == "vargrad"
    return [ENTRY_NAME[entry], str(N), str(D), str(PB), str(pn.mc), f"d4{pn.d4}", f"{'bs' if multi else 'ps'}{pn.gs}", f"ng{len(pn.groups)}",
            f"nrb{len(pn.blocks)}", f"{'ncb' if var else 'nqb'}{pn.nq}", f"gran{pn.gran}", f"s{pn.S}", f"chunk{pn.chunk}"]


def case_form(c):
    return deriv_form(c.entry, c.N, c.D, c.P, c.M)


def case_lines(c):
    return [form_words(c.entry, c.N, c.D, c.P, pn) for pn in case_form(c)]


# ---- operands --------------------------------------------------------------------------------------------------------------
_ops = {}


def sr_case(c, M=None):
    """The case of test_small_refs whose reference holds this case's outputs: its first period, B models of one output for a multi
    entry."""
    multi = is_multi(c)
    return SR.Case(c.group, _SR[c.entry][0], c.N, c.D, 1 if multi else c.P, ref_m(c) if M is None else M, c.P if multi else 1, c.pad, c.regime)


def case_operands(c):
    """The dict of test_small_refs.case_operands for the first period's queries: per model (lists) X (N, D) - one array for all
    models - ls (D), alpha (N, P | 1), W (Np, Np) (vargrad), sf2, kss; ys; Xq (ref_m, D).  Cached per case; never modified."""
    key = c._replace(group="", off=0, var=1, pad=0) if c.entry != "vargrad" else c._replace(group="", var=1, pad=0)
    if key in _ops:
        return _ops[key]
    rng = np.random.default_rng(zlib.crc32(repr(tuple(key[1:])).encode()))
    N, D, M = c.N, c.D, ref_m(c)
    B, P = (c.P, 1) if is_multi(c) else (1, c.P)
    Np = padded(N)
    X = rng.standard_normal((N, D))
    o = dict(X=[X] * B, ls=[], alpha=[], W=[], sf2=[], kss=[], noise=[0.0] * B, floor=SR.FLOOR)
    for b in range(B):
        o["ls"].append(rng.uniform(0.7, 2.5, D) * math.sqrt(D))
        o["alpha"].append(rng.uniform(0.5, 1.5, (N, P)) * rng.choice([-1.0, 1.0], (N, P)))
        o["sf2"].append(float(rng.uniform(0.6, 1.8)))
        if c.entry == "vargrad":
            W = np.tril(rng.standard_normal((Np, Np)) / math.sqrt(Np))
            W[np.arange(Np), np.arange(Np)] = np.abs(W.diagonal()) + 0.5 / math.sqrt(Np)
            W[N:, :N] = 0.0                                  # an inverse factor's padding rows (the docstring)
            o["W"].append(W)
    o["ym"] = np.zeros(B * P)
    o["ys"] = np.sort(rng.uniform(0.5, 3.0, B * P)) + 0.01 * np.arange(B * P)      # distinct
    Xq = rng.standard_normal((M, D))
    if M >= 2:
        Xq[0], Xq[1] = X[0], X[N - 1]
    if M >= 4:
        Xq[3] = Xq[2]
    if M >= 5:      # |x| < 8 and ls >= 0.7: the first coordinate alone is more than 60 length-scales from every row
        Xq[M - 1, 0] = 8.0 + 70.0 * max(float(ls[0]) for ls in o["ls"])
    o["Xq"] = Xq
    if c.entry == "vargrad":
        t = SR._sub_fp64(o, 0)
        if c.regime == "clip":      # between two neighbours of the sorted subtracted terms: half the variances clip, none is near
            s = np.sort(t)
            o["kss"].append(float(0.5 * (s[M // 2 - 1] + s[M // 2])))
        else:
            o["kss"].append(float(o["sf2"][0] + rng.uniform(0.0, 0.3) + t.max()))
    for v in o.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _ops[key] = o
    return o


def w_device_image(c):
    """The Np x ldw array the device holds for W: its lower triangle, exactly zero above the diagonal inside the band that gpk_trtri
    zeroes (up to the end of tile column i / 128 + GPK_ZERO_BAND_TILES - 1), NaN beyond the band and in the pitch columns."""
    Np = padded(c.N)
    W = case_operands(c)["W"][0]
    img = np.full((Np, Np + c.pad), np.nan)
    i, j = np.arange(Np)[:, None], np.arange(Np)[None, :]
    band = j < np.minimum(Np, (i // TILE + ZERO_BAND_TILES) * TILE)
    img[:, :Np] = np.where(j <= i, W, np.where(band, 0.0, np.nan))
    return img


def query_rows(c):
    """(M,) the row of the first period that query m repeats."""
    return np.arange(c.M) % period(c)


# ---- reference and bars ----------------------------------------------------------------------------------------------------
SLICE_BITS, SLICES, BIG_PRODUCT = 19, 4, 10 ** 8


SLICED_CALLS = [0]      # products that went through `sliced_matmul` (`sliced_products` keeps the count per reference)


def _slices(a, axis):
    """`a` (long double) as SLICES fp64 arrays that add up to it to 76 bits below the largest magnitude along `axis`: slice i holds
    integers of at most 20 bits times 2^(e - 19 (i + 1)), e per row (axis 1) or column (axis 0)."""
    mx = np.max(np.abs(a), axis=axis, keepdims=True).astype(np.float64)
    e = np.frexp(mx)[1] + 1
    rest, out = np.array(a, dtype=np.longdouble), []
    for i in range(SLICES):
        q = np.ldexp(np.longdouble(1.0), e - SLICE_BITS * (i + 1))
        s = np.rint(rest / q) * q
        out.append(s.astype(np.float64))
        rest = rest - s
    return out


def sliced_matmul(a, b):
    """a @ b for long-double matrices through fp64 products that are exact: a product of two slices is an integer of at most 38
    bits times one power of two per (row, column), so a sum of up to 8192 of them is exact in fp64 in any order (BLAS); the ten
    slice products down to 2^-76 of (row maximum) x (column maximum) are added in long double, the smallest first.  The two
    triangular products of the variance gradient's reference at Np = 2304 take 12 s in NumPy's long-double loop and 1 s here."""
    assert a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[0] <= 8192
    SLICED_CALLS[0] += 1
    sa, sb = _slices(a, 1), _slices(b, 0)
    tot = np.zeros((a.shape[0], b.shape[1]), dtype=np.longdouble)
    for lvl in range(SLICES - 1, -1, -1):
        for i in range(lvl + 1):
            tot += (sa[i] @ sb[lvl - i]).astype(np.longdouble)
    return tot


class _LD(np.ndarray):
    """A long-double array whose matrix products of BIG_PRODUCT multiplications and more go through `sliced_matmul`: the two
    products W K*^T and W^T V inside test_small_refs._model_reference, whose formulas stay where they are.  Which references take
    that path is pinned by test_which_references_take_the_sliced_product."""

    def __matmul__(self, other):
        a, b = np.asarray(self), np.asarray(other)
        if a.ndim == 2 and b.ndim == 2 and a.dtype == b.dtype == np.longdouble and a.shape[0] * a.shape[1] * b.shape[1] >= BIG_PRODUCT:
            return sliced_matmul(a, b).view(_LD)
        return np.matmul(a, b).view(_LD)


class FastHP(HP):
    """test_small_refs.HP in long double with the large products sliced; mpmath stays what it is."""

    def arr(self, a):
        r = HP.arr(self, a)
        return r.view(_LD) if self.kind == "longdouble" else r


def fast_hp():
    return FastHP(default_hp().kind)


_refs = {}
sliced_products = {}      # per cached reference: how many of its products were sliced


def _layout(c, a):
    """test_small_refs stacks the models in front: (B, M, P, ...) -> the entry's layout (M, P | B, ...); var, dvar: (M, ...)."""
    if is_multi(c):
        return np.moveaxis(a[:, :, 0], 0, 1)
    return a[0]


def deriv_reference(c, hp=None, keep=None):
    """{output: (value rounded to fp64, the value in the reference's format, scale, escale)} for the first period's queries, in the
    entry's layout: dmean (M, P | B, D), hess (M, P | B, D, D), var (M), dvar (M, D); "_raw" (M): kss - |W k*|^2 before the clip."""
    cached = hp is None and keep is None
    key = c._replace(group="", off=0, var=1, pad=0)
    if cached and key in _refs:
        return _refs[key]
    sc = sr_case(c)
    before = SLICED_CALLS[0]
    r = SR.small_reference(sc, ops=case_operands(c), hp=fast_hp() if hp is None else hp, keep=None if keep is None else [keep] * sc.B)
    res = {k: tuple(_layout(c, a) for a in r[k]) for k in _SR[c.entry][1]}
    if "_raw" in r:
        res["_raw"] = r["_raw"][0]
    if cached:
        _refs[key] = res
        sliced_products[key] = SLICED_CALLS[0] - before
    return res


def case_chains(c):
    """{output: the longest chain over the call's panels}."""
    forms = case_form(c)
    return {k: max(pn.chain[k] for pn in forms) for k in forms[0].chain}


def case_bars(c, ref=None):
    """{output: bar array over the first period}: 2^-53 (chain scale + escale)."""
    ref = deriv_reference(c) if ref is None else ref
    chains = case_chains(c)
    return {k: U * (chains[k] * ref[k][2] + ref[k][3]) for k in _SR[c.entry][1]}


def error_ratios(hp, got64, ref_entry, bar):
    """|got - reference| / bar per entry, the difference taken in the reference's format."""
    return ratio(hp.f64(np.abs(hp.arr(got64) - ref_entry[1])), bar)


def fp64_outputs(c, variant=0, keep=None):
    """Every output of the entry in plain fp64 NumPy (test_small_refs.fp64_outputs: three summation orders), in the entry's layout."""
    sc = sr_case(c)
    got = SR.fp64_outputs(sc, case_operands(c), variant, None if keep is None else [keep] * sc.B)
    return {k: _layout(c, got[k]) for k in _SR[c.entry][1]}


# ---- host tests --------------------------------------------------------------------------------------------------------------
def test_mirror_at_the_switch_points():
    f = deriv_form
    one = lambda *a: f(*a)[0]
    # gran at M = 512 | 513 and N = 16384 | 16385: N = 300, one group: nqb 2 | 3, S = 1024 | 683 -> 10 chunks of 32 | 3 of 128
    assert [(p.gran, p.S, p.chunk) for p in (one("grad", 300, 1, 1, 512), one("grad", 300, 1, 1, 513))] == [(32, 10, 32), (128, 3, 128)]
    assert [(p.gran, p.S, p.chunk) for p in (one("grad", 16384, 1, 1, 1), one("grad", 16385, 1, 1, 1))] == [(32, 512, 32), (128, 129, 128)]
    # output groups: P = 4 | 5 | 8 | 9 | 13
    assert [(one("grad", 9, 1, p, 1).gs, one("grad", 9, 1, p, 1).groups) for p in (4, 5, 8, 9, 13)] == \
        [(4, [(0, 4)]), (3, [(0, 3), (3, 2)]), (4, [(0, 4), (4, 4)]), (3, [(0, 3), (3, 3), (6, 3)]), (4, [(0, 4), (4, 4), (8, 4), (12, 1)])]
    assert [(one("grad_multi", 9, 1, b, 1).gs, len(one("grad_multi", 9, 1, b, 1).groups)) for b in range(1, 9)] == \
        [(1, 1), (2, 1), (3, 1), (4, 1), (3, 2), (3, 2), (4, 2), (4, 2)]
    assert one("grad_multi", 9, 1, 5, 1).groups == [(0, 3), (3, 2)] and one("grad_multi", 9, 1, 7, 1).groups == [(0, 4), (4, 3)]
    # d4 at D = 4 | 5 | 8 | 9 | 12 | 13, and the Hessian's row blocks with their live rows
    assert [one("grad", 9, d, 1, 1).d4 for d in (4, 5, 8, 9, 12, 13)] == [1, 2, 2, 3, 3, 4]
    assert [one("hess", 9, d, 3, 1).blocks for d in (4, 5, 8, 9, 12, 13, 14, 16)] == \
        [[(0, 4, 4)], [(0, 8, 5)], [(0, 8, 8)], [(0, 8, 8), (8, 12, 1)], [(0, 8, 8), (8, 12, 4)], [(0, 9, 9), (9, 13, 4), (13, 16, 0)],
         [(0, 9, 9), (9, 13, 4), (13, 16, 1)], [(0, 9, 9), (9, 13, 4), (13, 16, 3)]]
    assert [one("hess_multi", 9, d, 3, 1).blocks for d in (4, 5, 9, 13, 15)] == \
        [[(0, 4, 4)], [(0, 5, 5), (5, 8, 0)], [(0, 7, 7), (7, 10, 2), (10, 12, 0)], [(0, 7, 7), (7, 10, 3), (10, 12, 2), (12, 14, 1), (14, 16, 0)],
         [(0, 7, 7), (7, 10, 3), (10, 12, 2), (12, 14, 2), (14, 16, 1)]]
    # the Hessian's groups: up to four outputs at D <= 4, one above; models in fours at D <= 4, in twos above (B = 3: the second is masked)
    assert [(one("hess", 9, d, p, 1).gs, len(one("hess", 9, d, p, 1).groups)) for d, p in ((4, 5), (4, 16), (5, 3), (16, 16))] == \
        [(3, 2), (4, 4), (1, 3), (1, 16)]
    assert one("hess_multi", 9, 5, 3, 1).groups == [(0, 2), (2, 1)] and one("hess_multi", 9, 4, 7, 1).groups == [(0, 4), (4, 3)]
    # the Hessian's panel: P = D = 16: 2^28 / (16 * 137 * 8) = 15307 -> 59 * 256 = 15104; B = 5, D = 16: 48984 -> 48896; small blocks: 65536
    assert one("hess", 33, 16, 16, 1).panel == 15104 and one("hess_multi", 33, 16, 5, 1).panel == 48896 and one("hess", 33, 4, 4, 1).panel == 65536
    assert [(p.m0, p.mc, p.gran) for p in f("hess", 33, 16, 16, 15105)] == [(0, 15104, 128), (15104, 1, 32)]
    # capS: M = 8192, P = D = 16: nqb 32, 48 groups x blocks: S = 2 by the grid, 3 by the rows, 1 by 2^28 / (8192 * 16 * 137 * 8) = 1.87
    p = one("hess", 300, 16, 16, 8192)
    assert (p.capS, p.S, p.chunk, p.rounds, p.tail) == (1, 1, 384, 3, 44)
    # chunks of several rounds: M = 20000, P = 16: nqb 79 x 4 groups: S = 7 -> chunk 143 -> 256: 4 chunks, the last 232 = 128 + 104
    p = one("grad", 1000, 1, 16, 20000)
    assert (p.S, p.chunk, p.rounds, p.tail) == (4, 256, 2, 104)
    # two panels, the second with the other granularity
    assert [(p.m0, p.mc, p.nq, p.gran, p.S, p.chunk) for p in f("grad", 300, 1, 1, 65537)] == [(0, 65536, 256, 128, 3, 128), (65536, 1, 1, 32, 10, 32)]
    # the variance gradient: 64-row chunks until N M reaches 2e7: N = 640: ncb 228 -> S = 9 of 10 -> chunk 72 -> 128
    assert [(p.nq, p.S, p.chunk, p.rounds) for p in (one("vargrad", 640, 4, 1, 29056), one("vargrad", 640, 4, 1, 29057))] == \
        [(227, 10, 64, 1), (228, 5, 128, 2)]
    assert (one("vargrad", 2304, 9, 1, 129).S, one("vargrad", 2304, 9, 1, 129).chunk) == (36, 64)
    # chains, counted by hand at N = 300, M = 513 (three chunks of 128 rows)
    assert one("grad", 300, 9, 1, 513).chain == dict(dmean=4 + 128 + 3 + 3) and one("grad_multi", 300, 9, 1, 513).chain == dict(dmean=3 + 128 + 3 + 4)
    assert one("hess", 300, 9, 1, 513).chain == dict(hess=7 + 128 + 3 + 5) and one("hess_multi", 300, 9, 1, 513).chain == dict(hess=4 + 128 + 3 + 8)
    assert one("vargrad", 300, 9, 1, 513).chain == dict(var=2 * 385 + 1 + 64 + 5 + 1, dvar=385 + 384 + 4 + 64 + 5 + 2)
    assert case_lines(GROUPS["A"][19]) == [["mean_grad", "300", "1", "1", "65536", "d41", "ps1", "ng1", "nrb1", "nqb256", "gran128", "s3", "chunk128"],
                                           ["mean_grad", "300", "1", "1", "1", "d41", "ps1", "ng1", "nrb1", "nqb1", "gran32", "s10", "chunk32"]]
    assert case_lines(GROUPS["E"][11]) == [["mean_hess_multi", "129", "13", "7", "257", "d44", "bs2", "ng4", "nrb5", "nqb2", "gran32", "s5", "chunk32"]]
    assert case_lines(GROUPS["C"][7]) == [["var_grad", "2304", "9", "1", "129", "d43", "ps1", "ng1", "nrb1", "ncb2", "gran64", "s36", "chunk64"]]


def test_every_switch_point_is_a_case():
    forms = {c: case_form(c) for c in ALL_CASES}
    first = {c: f[0] for c, f in forms.items()}
    by = lambda e: {c: p for c, p in first.items() if c.entry == e}
    assert {(p.d4, p.gs) for p in by("grad").values()} == {(a, b) for a in range(1, 5) for b in range(1, 5)}
    assert {(p.d4, p.gs) for p in by("grad_multi").values()} == {(a, b) for a in range(1, 5) for b in range(1, 5)}
    assert {p.d4 for p in by("vargrad").values()} == {1, 2, 3, 4}
    seven = {(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (3, 1), (4, 1)}
    assert {(p.d4, p.gs) for p in by("hess").values()} == seven
    assert {(p.d4, p.gs) for p in by("hess_multi").values()} == {(1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (3, 2), (4, 2)}
    assert {c.D for c in GROUPS["A"]} == {1, 4, 5, 8, 9, 12, 13, 16} and {c.P for c in GROUPS["A"]} == {1, 2, 3, 4, 5, 7, 9, 13, 16}
    assert {1, 31, 32, 33, 127, 128, 129, 300, 16384, 16385} <= {c.N for c in GROUPS["A"]} and {1, 255, 256, 257, 512, 513} <= {c.M for c in GROUPS["A"]}
    assert {c.P for c in GROUPS["B"]} == set(range(1, 9)) and {c.P for c in GROUPS["E"]} == set(range(1, 9))
    assert {c.D for c in GROUPS["D"]} == {1, 2, 3, 4, 5, 8, 9, 12, 13, 14, 16} and {c.D for c in GROUPS["E"]} == {1, 4, 5, 8, 9, 12, 13, 15, 16}
    assert {c.P for c in GROUPS["D"] if c.D <= 4} == {1, 2, 3, 4, 5, 7, 16} and {c.P for c in GROUPS["D"] if c.D > 4} == {1, 3, 16}
    assert {1, 33, 129, 300} <= {c.N for c in GROUPS["D"]} and {1, 256, 257, 513} <= {c.M for c in GROUPS["D"]}
    assert any(c.P % 2 and c.P > 1 and c.D > 4 for c in GROUPS["E"])
    for g in "ABDE":      # both granularities, a group with a masked slot, two panels
        ps = [p for c in GROUPS[g] for p in forms[c]]
        assert {32, 128} <= {p.gran for p in ps} and any(n < p.gs for p in ps for _, n in p.groups)
        assert any(len(forms[c]) == 2 for c in GROUPS[g])
    # row blocks that are whole, partly filled and empty
    for g in "DE":
        bl = [b for c in GROUPS[g] for b in first[c].blocks]
        assert any(n == 0 for _, _, n in bl) and any(0 < n < r1 - r0 for r0, r1, n in bl) and any(n == r1 - r0 for r0, r1, n in bl)
    # several rounds with a ragged last one; the capS-bound chunk; the reduced panels
    assert any(p.rounds >= 2 and p.tail < JG_TJ and p.S > 1 for p in by("grad").values())
    assert any(p.capS == 1 and p.rounds == 3 for p in by("hess").values())
    assert any(p.panel == 15104 for p in by("hess").values()) and any(p.panel == 48896 for p in by("hess_multi").values())
    # the variance gradient
    C = GROUPS["C"]
    assert {128, 256, 640, 2304} <= {padded(c.N) for c in C} and any(c.N == padded(c.N) - 127 for c in C) and {1, 127, 128, 129, 300} <= {c.M for c in C}
    assert {0, 2} == {c.pad for c in C} and {0, 1} == {c.var for c in C} and any(c.regime == "clip" for c in C)
    assert any(p.rounds == 2 for p in by("vargrad").values()) and any(padded(c.N) > ZERO_BAND_TILES * TILE for c in C)
    assert len({c.entry for c in SEQUENCE}) == 5 and len(SEQUENCE) == 6
    assert all(not c.off or c.entry != "vargrad" for c in ALL_CASES) and sum(c.off for c in ALL_CASES) >= 8


@pytest.mark.parametrize("c", ALL_CASES, ids=case_id)
def test_operands_are_what_the_docstring_says(c):
    o = case_operands(c)
    M, B = ref_m(c), len(o["ls"])
    assert len({tuple(ls) for ls in o["ls"]}) == B and len(set(o["sf2"])) == B and len(set(o["ys"])) == o["ys"].size
    for b in range(B):
        assert (o["ls"][b] >= 0.7 * math.sqrt(c.D)).all() and (o["ls"][b] <= 2.5 * math.sqrt(c.D)).all()
        assert (np.abs(o["alpha"][b]) >= 0.5).all() and (np.abs(o["alpha"][b]) <= 1.5).all()
        K = SR._kstar64(o, b)[0]
        if M >= 5:
            assert not K[M - 1].any(), "the far query's kernel row is exactly zero"
            assert (K[:M - 1] > 0).all()
    assert np.abs(o["X"][0]).max() < 8.0
    if M >= 4:
        assert np.array_equal(o["Xq"][2], o["Xq"][3]) and np.array_equal(o["Xq"][0], o["X"][0][0]) and np.array_equal(o["Xq"][1], o["X"][0][c.N - 1])
    ref = deriv_reference(c)
    if M >= 5:
        for k in _SR[c.entry][1]:
            if k != "var":
                assert not ref[k][0][M - 1].any(), "every derivative at the far query is exactly zero"
    if c.entry == "vargrad":
        Np, W, img = padded(c.N), o["W"][0], w_device_image(c)
        assert not np.triu(W, 1).any() and (W.diagonal() > 0).all() and not W[c.N:, :c.N].any() and (W[:c.N, :c.N][np.tril_indices(c.N)] != 0).all()
        assert img.shape == (Np, Np + c.pad) and np.isnan(img[:, Np:]).all()
        i, j = np.tril_indices(Np)
        assert np.array_equal(img[i, j], W[i, j])
        for r in sorted({0, 127, Np - 128, Np - 1}):
            end = min(Np, (r // 128 + 16) * 128)
            assert not img[r, r + 1:end].any() and np.isnan(img[r, end:]).all()
        assert (np.isnan(img[:, :Np]).any()) == (Np > 2048)
    if c.regime == "clip":
        clipped = ref["_raw"] < o["floor"]
        assert 8 <= clipped.sum() <= M - 8 and np.array_equal(ref["var"][0][clipped], np.full(int(clipped.sum()), o["floor"]))
        assert (np.abs(ref["_raw"] - o["floor"]) > 1e3 * case_bars(c)["var"]).all(), "no variance sits at the clip"


@pytest.mark.parametrize("c", ALL_CASES, ids=case_id)
def test_fp64_numpy_in_any_order_stays_within_the_bars(c):
    hp, ref, bars = default_hp(), deriv_reference(c), case_bars(c)
    worst = 0.0
    for variant in range(3):
        got = fp64_outputs(c, variant)
        for k in _SR[c.entry][1]:
            r = float(np.max(error_ratios(hp, got[k], ref[k], bars[k])))
            worst = max(worst, r)
            assert r <= 1.0, (k, variant, r)
    print(f"{case_id(c)}: fp64 NumPy, three orders: largest error / bar {worst:.3f}")


@pytest.mark.parametrize("c", ALL_CASES, ids=case_id)
def test_a_lost_block_chunk_or_slot_leaves_the_bars(c):
    """32 training rows dropped from K* (every block up to N = 1024, else the first, the last and six seeded ones), one whole chunk of
    the first panel dropped (the first and the last), or the last slot of every group left out (its outputs would be 0).  Per cut and
    output: some entry moves by at least 100 bars, and so does the median query - the largest move among a query's entries, the
    median over the queries but the far one (and, for a clipped variance, but the clipped ones): the bars cannot hide a fault that
    hits only some query blocks or rows.  Not every single query can be asked to: query 1 is training row N - 1, whose own term in
    dmean is exactly 0, so at N = 33 or 129 the last block (that row alone) leaves it where it was.  fp64 differences: a
    sensitivity, not an accuracy."""
    bars = case_bars(c)
    full = fp64_outputs(c)
    outs = _SR[c.entry][1]
    pn = case_form(c)[0]
    M, nb = ref_m(c), _ceil(c.N, 32)
    blocks = list(range(nb)) if nb <= 32 else sorted({0, nb - 1, *np.random.default_rng(3).choice(nb, 6, replace=False).tolist()})
    cuts = [(32 * b, 32 * b + 32) for b in blocks]
    if pn.S > 1:
        cuts += [(0, pn.chunk), ((pn.S - 1) * pn.chunk, c.N)]
    near = np.arange(M) < (M - 1 if M >= 5 else M)
    least, least_median = math.inf, math.inf
    for lo, hi in cuts:
        keep = np.ones(c.N)
        keep[lo:hi] = 0.0
        got = fp64_outputs(c, keep=keep)
        for k in outs:
            live = near & (full[k] > SR.FLOOR) & (got[k] > SR.FLOOR) if k == "var" and c.regime == "clip" else near
            per_query = ratio(np.abs(got[k] - full[k]), bars[k])[live].reshape(int(live.sum()), -1).max(axis=1)
            r, med = float(per_query.max()), float(np.median(per_query))
            least, least_median = min(least, r), min(least_median, med)
            assert r >= 100.0 and med >= 100.0, (k, lo, hi, r, med)
    if c.entry != "vargrad":
        k = outs[0]
        for p0, n in pn.groups:
            per_query = ratio(np.abs(full[k][:, p0 + n - 1]), bars[k][:, p0 + n - 1])[near].reshape(int(near.sum()), -1).max(axis=1)
            r, med = float(per_query.max()), float(np.median(per_query))
            least, least_median = min(least, r), min(least_median, med)
            assert r >= 100.0 and med >= 100.0, (k, "slot", p0 + n - 1, r, med)
    print(f"{case_id(c)}: a lost block, chunk or slot: at least {least:.2e} bars somewhere, {least_median:.2e} at the median query")


def test_sliced_product_is_the_long_double_product():
    if default_hp().kind != "longdouble":
        pytest.skip("the sliced product serves the long-double format only")
    rng = np.random.default_rng(11)
    a = (rng.standard_normal((70, 900)) * np.exp(rng.uniform(-12, 0, (70, 900)))).astype(np.longdouble) * (1 + np.longdouble(2.0) ** -60)
    b = (rng.standard_normal((900, 50)) * np.exp(rng.uniform(-12, 0, (900, 50)))).astype(np.longdouble) * (1 - np.longdouble(2.0) ** -58)
    plain, mag = a @ b, (np.abs(a) @ np.abs(b)).astype(np.float64)
    assert np.max(np.abs(sliced_matmul(a, b) - plain).astype(np.float64) / mag) <= 900 * 2.0 ** -63      # the plain loop's own rounding
    ints = np.rint(rng.standard_normal((40, 600)) * 1000).astype(np.longdouble)
    assert np.array_equal(sliced_matmul(ints, ints.T.copy()), ints @ ints.T)
    big = fast_hp().arr(np.ones((500, 500)))
    assert isinstance(big @ big, _LD) and np.array_equal(np.asarray(big @ big), np.full((500, 500), 500.0, dtype=np.longdouble))


def test_which_references_take_the_sliced_product():
    """Only the variance gradient's two products W K*^T and W^T V, and only from Np N M = 1e8 on (N = 640 with M = 300 or a whole
    period, Np = 2304); every other reference is NumPy's own long-double arithmetic throughout."""
    if default_hp().kind != "longdouble":
        pytest.skip("the sliced product serves the long-double format only")
    for c in ALL_CASES:
        deriv_reference(c)
        big = c.entry == "vargrad" and padded(c.N) * c.N * ref_m(c) >= BIG_PRODUCT
        assert sliced_products[c._replace(group="", off=0, var=1, pad=0)] == (2 if big else 0), case_id(c)
    assert [case_id(c) for c in GROUPS["C"] if padded(c.N) * c.N * ref_m(c) >= BIG_PRODUCT] == \
        ["C-vargrad-N640-D13-P1-M300", "C-vargrad-N2304-D9-P1-M129", "C-vargrad-N640-D4-P1-M29057"]


def test_mpmath_path_agrees_with_long_double():
    pytest.importorskip("mpmath")
    if np.finfo(np.longdouble).eps > 2.0 ** -63:
        pytest.skip("long double is no wider than fp64 here: mpmath is the reference already")
    for c in (_c("X", "vargrad", 40, 3, 1, 6), _c("X", "hess", 40, 3, 2, 6), _c("X", "grad_multi", 40, 5, 3, 6)):
        a, b = deriv_reference(c, hp=HP("mpmath")), deriv_reference(c, hp=HP("longdouble"))
        for k in _SR[c.entry][1]:
            assert np.max(ratio(np.abs(a[k][0] - b[k][0]), a[k][2])) <= 2.0 ** -52, k
            assert np.array_equal(a[k][2], b[k][2])
