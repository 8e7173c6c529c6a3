"""Host side of tests/test_gpu_small_forms.py: the cases, their operands, an extended-precision reference, the mirror of
gpk_small_launch's launch rule and the bars of the small-batch serving kernels (gpk_small.hip) - nothing here needs a GPU.

Operands (`case_operands`), from a seed derived from the case; every model of a batch has its own:
* X standard normal; length-scales per model and feature in [0.7, 2.5] sqrt(D) (most squared distances below about 20);
* alpha: random signs, magnitude in [0.5, 1.5];
* W: a dense random lower-triangular Np x Np matrix, entries N(0, 1) / sqrt(Np), diagonal positive - the inverse factor of nothing:
  every entry of its lower triangle, rows N .. Np - 1 included, counts in V = W K*^T;
* kss, sf2, noise, y_mean, y_std differ per model and output;
* queries: standard normal; query 0 is training row 0 and query 1 training row N - 1 of model 0 (M >= 2), queries 2 and 3 are
  the same row (M >= 4), and the last query (M >= 5) lies more than 60 length-scales from every training row of every model: its
  kernel row is exactly 0 in fp64, its mean y_mean and its variance kss.  Regime "clip": kss lies between the subtracted terms
  of the queries, so that about half of the variances clip at floor_.

Reference (`small_reference`): the formulas of include/gpk.h, literally, in np.longdouble (eps 2^-64; where the platform's
long double is no wider than that, mpmath at 80 bits through object arrays - `HP` - the same code).  K* by exact differences of
inputs divided by the length-scales, rows N .. Np - 1 zero; mean = y_mean + y_std (K* alpha); var = max(kss - |W k*|^2, floor);
cov = K(Xq, Xq) + noise [row = column] - (W K*^T)^T (W K*^T); dmean; dvar = -2 sum_j k u c, c = W^T (W k*); hess = y_std /
(ls_d ls_e) (T - [d = e] S).  Every output comes with its scale - the same expression, every summand replaced by its absolute
value (a difference x / ls - q / ls counts |x / ls| + |q / ls|: both quotients are rounded) - and its escale: the scale with every
kernel value weighted by the exponential's term of its own pair (both in fp64: they are bars, not values).

Bars: bar = 2^-53 (chain scale + escale), first order.  chain: the longest chain of rounding operations behind the output, counted
from the kernels' loops by `small_form` (an fp64 MFMA counted as four chained fused multiply-adds).  The exponential's term of a
pair, in units of 2^-53: EXP_ULPS = 3 for gpk_exp_neg itself (gpk_math.h: Taylor degree 13 on |r| <= ln2 / 2, truncation 4e-18 =
0.04; the two fused steps of the reduction 0.7; Horner's last step 1 and the earlier ones damped by |r| <= 0.35, 1.54 in all), plus
the rounding of its argument amplified by d^2 / 2: sum_d |df_d| (|df_d| + |q_d / ls_d| + |x_d / ls_d|) + D d^2 / 2.  Nothing in a
bar is taken from a GPU result.

Shapes: gpk_padded rounds N up to 128, so no call has Np = 576; the nine-chunk row blocks (rows 512 .. 575) are reached at Np =
640, whose last row blocks have ten chunks - still one pipelined round (waves 0 and 1 take a second chunk, none a third).

Host tests: the mirror at hand-counted switch points; plain fp64 NumPy in three orders within every bar - largest ratio of the
fp64 error to the bar over all cases and outputs: 0.047 (A-predict-N128-D1-P15-M9; the Hessians up to 0.042, the variances and
covariances below 0.02); a true inverse Cholesky factor reproduces the closed-form posterior; any
32-row block of training rows removed leaves a bar of every output by at least 100 x (measured: at least 1e6 x); the mpmath path agrees with
the long-double path on a small case.
"""
import math
import zlib
from collections import namedtuple

import numpy as np
import pytest

Case = namedtuple("Case", "group entry N D P M B pad regime")
Form = namedtuple("Form", "call B Np M ga gb nmb nch v_rounds idle_waves fm_parts fm_passes fj_passes cov_groups cov_top_rounds var_share_rounds "
                          "rc wtv_passes hess_rows hess_rounds hess_groups hess_slice slices chains")

U = 2.0 ** -53
EXP_ULPS = 3.0
FLOOR = 1e-10
SQ, SJ, SR, CG, HJ, VW = 32, 32, 16, 16, 32, 8
WTV_MAX_ROW_CHUNKS, GRG, GT = 4, 16, 512
HESS_SLICE_ENTRIES = 512
# entry -> (the launch routine's call, outputs)
ENTRIES = {
    "predict": ("predict", ("mean",)), "predict_var": ("predict", ("mean", "var")),
    "cov": ("cov", ("mean", "cov")),
    "grad": ("grad", ("mean", "dmean")), "grad_var": ("grad", ("mean", "var", "dmean", "dvar")),
    "hess": ("hess", ("mean", "dmean", "hess")),
}


def call_of(c):
    return ENTRIES[c.entry.replace("multi_", "")][0]


def outputs_of(c):
    return ENTRIES[c.entry.replace("multi_", "")][1]


def padded(n):
    return (n + 127) // 128 * 128


def _c(group, entry, N, D, P, M, B=1, pad=0, regime="plain"):
    return Case(group, entry, N, D, P, M, B, pad, regime)


GROUPS = {
    # mean only: N in {1, 31, 32, 33, 128, 129, 1000}, D in {1, 9, 16}, M P across 64, 128, 256 and at 512; M = 33, 64: two chunks
    "A": [_c("A", "predict", 1, 1, 1, 1), _c("A", "predict", 31, 9, 16, 4), _c("A", "predict", 32, 16, 13, 5),
          _c("A", "predict", 33, 9, 16, 8), _c("A", "predict", 128, 1, 15, 9), _c("A", "predict", 129, 16, 16, 16),
          _c("A", "predict", 1000, 9, 16, 17), _c("A", "predict", 1000, 16, 16, 32), _c("A", "predict", 129, 9, 16, 33),
          _c("A", "predict", 33, 1, 16, 64)],
    # mean + variance: Np = 128 (N = Np and N = Np - 127), 640 (9 and 10 chunks), 1152 (18), 2176 (136 shares); M in {1, 16, 17, 32}
    "B": [_c("B", "predict_var", 128, 9, 1, 1), _c("B", "predict_var", 1, 1, 1, 16, pad=2), _c("B", "predict_var", 640, 9, 3, 17),
          _c("B", "predict_var", 513, 16, 1, 32, pad=2), _c("B", "predict_var", 1152, 9, 1, 16, pad=2),
          _c("B", "predict_var", 1100, 16, 2, 32), _c("B", "predict_var", 2100, 9, 1, 17, pad=2),
          _c("B", "predict_var", 300, 9, 1, 32, regime="clip")],
    # covariance: Np in {128, 256, 384, 2176} = half a group, one, one and a half, nine; M in {1, 16, 17, 32}; P in {1, 3}
    "C": [_c("C", "cov", 100, 9, 1, 1), _c("C", "cov", 128, 16, 3, 16, pad=2), _c("C", "cov", 256, 9, 1, 17),
          _c("C", "cov", 200, 1, 3, 32, pad=2), _c("C", "cov", 384, 9, 1, 32), _c("C", "cov", 300, 16, 3, 16),
          _c("C", "cov", 2100, 9, 1, 17, pad=2), _c("C", "cov", 2176, 9, 3, 32)],
    # gradients: mean + Jacobian at M P D = 1, 1024, 1040, 8192; all four at Np = 128 (rc 4), 2048 (rc 2), 2176 (rc 1); M D = 512
    "D": [_c("D", "grad", 33, 1, 1, 1), _c("D", "grad", 129, 16, 2, 32), _c("D", "grad", 100, 16, 13, 5), _c("D", "grad", 300, 16, 16, 32),
          _c("D", "grad_var", 100, 9, 2, 1), _c("D", "grad_var", 128, 16, 1, 32, pad=2), _c("D", "grad_var", 2048, 9, 1, 16),
          _c("D", "grad_var", 2100, 9, 3, 17, pad=2)],
    # Hessian: N = 1 (three empty workgroups), 33, 129; Np = 2176 (34 rows: 32 + 2), 4096 (64 rows); D = 1 with M P = 512 (2 slices);
    # D = 16, P = 2, M = 32 (slices of 3 pairs straddle queries); D = 10, P = 6, M = 25
    "E": [_c("E", "hess", 1, 9, 1, 1), _c("E", "hess", 33, 10, 6, 25), _c("E", "hess", 129, 16, 2, 32), _c("E", "hess", 2100, 9, 1, 4),
          _c("E", "hess", 4000, 3, 2, 5), _c("E", "hess", 100, 1, 16, 32)],
    # model batch: B in {2, 8}; predict, cov and hess at Np in {128, 384}; grad at B = 8 with Np = 256 (rc 2) and 512 (rc 1)
    "F": [_c("F", "multi_predict", 129, 9, 1, 32, B=8), _c("F", "multi_predict_var", 100, 9, 1, 17, B=2),
          _c("F", "multi_predict_var", 300, 16, 1, 16, B=8, pad=2), _c("F", "multi_cov", 128, 9, 1, 32, B=8),
          _c("F", "multi_cov", 300, 16, 1, 17, B=2, pad=2), _c("F", "multi_hess", 300, 10, 1, 25, B=2),
          _c("F", "multi_hess", 100, 16, 1, 32, B=8), _c("F", "multi_grad", 100, 9, 1, 5, B=2),
          _c("F", "multi_grad_var", 200, 9, 1, 17, B=8), _c("F", "multi_grad_var", 512, 16, 1, 32, B=8, pad=2)],
}
ALL_CASES = [c for g in GROUPS.values() for c in g]
# the sequence of group G on one handle: cov (B = 8), hess, grad (all four), cov (B = 1), predict twice
SEQUENCE = [GROUPS["F"][3], GROUPS["E"][1], GROUPS["D"][5], GROUPS["C"][3], GROUPS["B"][2], GROUPS["B"][2]]


def case_id(c):
    return f"{c.group}-{c.entry}-N{c.N}-D{c.D}-P{c.P}-M{c.M}" + (f"-B{c.B}" if c.B > 1 else "") + (f"-ldw+{c.pad}" if c.pad else "") + \
        ("" if c.regime == "plain" else "-" + c.regime)


# ---- the launch rule of gpk_small_launch, restated ---------------------------------------------------------------------
def hess_slice(D):
    return max(1, HESS_SLICE_ENTRIES // (D * (D + 1) // 2 + 1))


def _ceil(a, b):
    return -(-a // b)


def small_form(call, N, D, P, M, B=1):
    """The launches of one gpk_small_launch (M <= 32) and the longest chain of rounding operations behind each output."""
    assert 1 <= M <= SQ and call in ("predict", "cov", "grad", "hess")
    Np = padded(N)
    ga, gb = Np // SJ, Np // SR
    nmb = 1 if M <= 16 else 2
    nch = Np // 64                                   # the last row block of small_v_rows: min(Np, its diagonal rounded up to 64) / 64
    per_wave = _ceil(nch, VW)                        # chunks of the busiest wave (wave 0)
    v_rounds = _ceil(per_wave, 2)                    # passes of the two-chunk pipeline: 2 and more reload f0 (n2)
    MP, MPD = M * P, M * P * D
    fm_parts = 4 if 4 * MP <= 256 else 2 if 2 * MP <= 256 else 1
    fm_passes = _ceil(MP, 256 // fm_parts)
    ng = _ceil(gb, CG)
    rc = min(WTV_MAX_ROW_CHUNKS, max(1, 256 // (gb * B)))
    rows = max(32, Np // 64)
    hg = _ceil(Np, rows)
    # chains.  K*: sf2 * exp, one rounding (the exponential's own term is in escale)
    k = 1
    mean = k + SJ + _ceil(ga, fm_parts) + (fm_parts - 1) + 2          # 32 fma, the part's shares, the parts, y_std *, y_mean +
    v = k + 4 * 16 * per_wave + VW                                     # 16 MFMAs of depth 4 per chunk, the 8 waves' partials
    var = 2 * v + 1 + 16 + _ceil(gb, 2 * VW) + 2 * VW + 1              # v * v, 16 rows, the part's shares, 16 parts, kss -
    cov = 2 * v + 16 + min(CG, gb) + ng + 2                            # 16 fma, the group's shares, the groups, kv, kv - s
    dmean = k + 4 + SJ + ga + 2                                        # k alpha, x / ls (or q / ls), -, fma; shares; y_std / ls, *
    span = _ceil(_ceil(Np, rc), GRG) * GRG
    cc = v + span // GRG + GRG                                         # C = W^T V: the thread's rows, the 16 row groups
    ns = gb * rc
    dvar = max(cc, k) + 1 + 3 + 16 + _ceil(ns, 2) + 1 + 2              # K* C, x / ls, -, fma of 16; the half's shares, halves; -2 / ls, *
    hess = k + 7 + _ceil(rows, HJ) * HJ + hg + 1 + 3                   # k alpha, (q / ls - x / ls) twice, *, fma; rows; groups; - S; y_std / (ls ls) *
    grad_all = call == "grad"
    return Form(call, B, Np, M, ga, gb, nmb, nch, v_rounds, max(0, VW - nch), fm_parts, fm_passes,
                {"predict": 0, "cov": 0, "grad": _ceil(MPD, 4 * 256), "hess": _ceil(MPD, 4 * 256)}[call], ng, _ceil(ng, 8),
                _ceil(_ceil(gb, 2 * VW), 8), rc if grad_all else 0, _ceil(M * D, GT // 2) if grad_all else 0, rows, _ceil(rows, HJ), hg,
                hess_slice(D), _ceil(MP, hess_slice(D)) if call == "hess" else 0,
                dict(mean=mean, var=var, cov=cov, dmean=dmean, dvar=dvar, hess=hess))


def form_words(c, M=None, factors=None):
    """The words of the library's GPKSMALL line (option gram_log) for one launch sequence of a case (M: the chunk's queries)."""
    M = min(c.M, SQ) if M is None else M
    call = call_of(c)
    f = small_form(call, c.N, c.D, c.P, M, c.B)
    factors = ("var" in outputs_of(c) or call == "cov") if factors is None else factors
    return [call, str(c.B), "1", str(f.Np), str(M), str(c.D), str(c.P), f"ga{f.ga}", f"gb{f.gb}", f"nmb{f.nmb if factors else 0}",
            f"rc{f.rc if factors and call == 'grad' else 0}", f"hg{f.hess_groups if call == 'hess' else 0}", f"sl{f.slices}"]


def case_lines(c):
    """Every GPKSMALL line of the case's call: one per chunk of 32 queries."""
    return [form_words(c, min(SQ, c.M - m0)) for m0 in range(0, c.M, SQ)]


# ---- operands ----------------------------------------------------------------------------------------------------------
_ops = {}


def case_operands(c):
    """dict: Xq (M, D), floor, ym / ys (B P), and per model (lists of B): X (N, D), ls (D), alpha (N, P), W (Np, Np) lower triangular,
    sf2, kss, noise.  Cached per case; never modified."""
    if c in _ops:
        return _ops[c]
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c[2:])).encode()))      # (not the group or the entry: the same shape, the same operands)
    N, D, P, M, B = c.N, c.D, c.P, c.M, c.B
    Np = padded(N)
    o = dict(X=[], ls=[], alpha=[], W=[], sf2=[], kss=[], noise=[], floor=FLOOR)
    for b in range(B):
        o["X"].append(rng.standard_normal((N, D)))
        o["ls"].append(rng.uniform(0.7, 2.5, D) * math.sqrt(D))
        o["alpha"].append(rng.uniform(0.5, 1.5, (N, P)) * rng.choice([-1.0, 1.0], (N, P)))
        W = np.tril(rng.standard_normal((Np, Np)) / math.sqrt(Np))
        W[np.arange(Np), np.arange(Np)] = np.abs(W.diagonal()) + 0.5 / math.sqrt(Np)
        o["W"].append(W)
        o["sf2"].append(float(rng.uniform(0.6, 1.8)))
        o["noise"].append(float(rng.uniform(0.01, 0.2)))
    o["ym"] = rng.uniform(-2.0, 2.0, B * P)
    o["ys"] = rng.uniform(0.5, 3.0, B * P)
    Xq = rng.standard_normal((M, D))
    if M >= 2:
        Xq[0], Xq[1] = o["X"][0][0], o["X"][0][N - 1]
    if M >= 4:
        Xq[3] = Xq[2]
    if M >= 5:      # |x| < 8 and ls >= 0.7: the first coordinate alone is more than 60 length-scales from every row
        Xq[M - 1, 0] = 8.0 + 70.0 * max(float(ls[0]) for ls in o["ls"])
    o["Xq"] = Xq
    for b in range(B):
        t = _sub_fp64(o, b)
        if c.regime == "clip":      # between the 16th and the 17th of the sorted subtracted terms: half the variances clip, none is near
            s = np.sort(t)
            o["kss"].append(float(0.5 * (s[M // 2 - 1] + s[M // 2])))
        else:
            o["kss"].append(float(o["sf2"][b] + rng.uniform(0.0, 0.3) + t.max()))
    for v in o.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _ops[c] = o
    return o


def _kstar64(o, b, keep=None, order=None):
    Xs, Qs = o["X"][b] / o["ls"][b], o["Xq"] / o["ls"][b]
    df = Qs[:, None, :] - Xs[None, :, :]
    d2 = np.zeros(df.shape[:2])
    for d in (range(df.shape[2]) if order is None else order(df.shape[2])):
        d2 = d2 + df[:, :, d] * df[:, :, d]
    K = o["sf2"][b] * np.exp(-0.5 * d2)
    if keep is not None:
        K = K * keep[None, :]
    return K, df, Xs, Qs


def _sub_fp64(o, b):
    K, _, _, _ = _kstar64(o, b)
    N = K.shape[1]
    V = o["W"][b][:, :N] @ K.T
    return (V * V).sum(axis=0)


# ---- extended precision: long double, or mpmath through object arrays ---------------------------------------------------
class HP:
    """The number format of the reference.  'longdouble' needs eps <= 2^-63; 'mpmath' works at 80 bits everywhere."""

    def __init__(self, kind):
        self.kind = kind
        if kind == "mpmath":
            import mpmath
            self.mp = mpmath.mp.clone()
            self.mp.prec = 80
            self._exp = np.frompyfunc(self.mp.exp, 1, 1)
            self._conv = np.frompyfunc(lambda x: self.mp.mpf(float(x)), 1, 1)

    def arr(self, a):
        a = np.asarray(a, dtype=np.float64)
        return a.astype(np.longdouble) if self.kind == "longdouble" else self._conv(a)

    def exp(self, a):
        return np.exp(a) if self.kind == "longdouble" else self._exp(a)

    def zeros(self, shape):
        return self.arr(np.zeros(shape))

    def f64(self, a):
        return np.asarray(a, dtype=np.longdouble).astype(np.float64) if self.kind == "longdouble" else np.array(
            np.frompyfunc(float, 1, 1)(a), dtype=np.float64)


def default_hp():
    return HP("longdouble" if np.finfo(np.longdouble).eps <= 2.0 ** -63 else "mpmath")


def _model_reference(hp, c, o, b, outs, keep=None):
    """Model b of a case: {output: (value in the reference's format, scale fp64, escale fp64)}.  keep: a 0 / 1 weight per training
    row (a dropped row leaves K*, so every sum)."""
    N, D, P, M = c.N, c.D, c.P, c.M
    Np = padded(N)
    ls, sf2 = hp.arr(o["ls"][b]), hp.arr(o["sf2"][b])
    Xs, Qs = hp.arr(o["X"][b]) / ls, hp.arr(o["Xq"]) / ls
    ym, ys = hp.arr(o["ym"][b * P:(b + 1) * P]), hp.arr(o["ys"][b * P:(b + 1) * P])
    alpha = hp.arr(o["alpha"][b])
    df = Qs[:, None, :] - Xs[None, :, :]                       # (M, N, D): q / ls - x / ls
    d2 = (df * df).sum(axis=2)
    K = sf2 * hp.exp(d2 * hp.arr(-0.5))
    if keep is not None:
        K = K * hp.arr(keep)[None, :]
    # fp64 companions: |.| of everything, and the exponential's term of every pair
    ls64, sf264, ym64, ys64, a64 = o["ls"][b], o["sf2"][b], np.abs(o["ym"][b * P:(b + 1) * P]), np.abs(o["ys"][b * P:(b + 1) * P]), np.abs(o["alpha"][b])
    K64, df64, Xs64, Qs64 = _kstar64(o, b, keep)
    ad = np.abs(Qs64)[:, None, :] + np.abs(Xs64)[None, :, :]   # |q / ls| + |x / ls|
    ek = EXP_ULPS + (np.abs(df64) * (np.abs(df64) + ad)).sum(axis=2) + 0.5 * D * (df64 * df64).sum(axis=2)
    KE64 = K64 * ek
    res = {}
    S = K @ alpha
    res["mean"] = (ym + ys * S, ym64 + ys64 * (K64 @ a64), ys64 * (KE64 @ a64))
    if "dmean" in outs:
        val = hp.zeros((M, P, D))
        sc, es = np.zeros((M, P, D)), np.zeros((M, P, D))
        for d in range(D):
            val[:, :, d] = (ys / ls[d]) * ((K * -df[:, :, d]) @ alpha)
            sc[:, :, d] = (ys64 / ls64[d]) * ((K64 * ad[:, :, d]) @ a64)
            es[:, :, d] = (ys64 / ls64[d]) * ((KE64 * ad[:, :, d]) @ a64)
        res["dmean"] = (val, sc, es)
    if "hess" in outs:
        val = hp.zeros((M, P, D, D))
        sc, es = np.zeros((M, P, D, D)), np.zeros((M, P, D, D))
        S64, SE64 = K64 @ a64, KE64 @ a64
        for d in range(D):
            for e in range(d + 1):
                t = (K * df[:, :, d] * df[:, :, e]) @ alpha
                w = ad[:, :, d] * ad[:, :, e]
                ts, te = (K64 * w) @ a64, (KE64 * w) @ a64
                if d == e:
                    t, ts, te = t - S, ts + S64, te + SE64
                f, f64 = ys / (ls[d] * ls[e]), ys64 / (ls64[d] * ls64[e])
                val[:, :, d, e] = val[:, :, e, d] = f * t
                sc[:, :, d, e] = sc[:, :, e, d] = f64 * ts
                es[:, :, d, e] = es[:, :, e, d] = f64 * te
        res["hess"] = (val, sc, es)
    if "var" in outs or "cov" in outs or "dvar" in outs:
        W = hp.arr(o["W"][b][:, :N])                           # rows N .. Np - 1 of K* are zero: only the first N columns of W count
        Wa = np.abs(o["W"][b][:, :N])
        V, Va, VE = W @ K.T, Wa @ K64.T, Wa @ KE64.T           # (Np, M)
        if "var" in outs:
            kss = o["kss"][b]
            sub = (V * V).sum(axis=0)
            raw = hp.arr(kss) - sub
            val = np.where(raw > hp.arr(o["floor"]), raw, hp.arr(o["floor"]) + 0 * raw)
            res["var"] = (val, abs(kss) + (Va * Va).sum(axis=0), 2.0 * (Va * VE).sum(axis=0))
            res["_raw"] = hp.f64(raw)
        if "cov" in outs:
            dq = Qs[:, None, :] - Qs[None, :, :]
            kq = sf2 * hp.exp((dq * dq).sum(axis=2) * hp.arr(-0.5))
            dq64 = Qs64[:, None, :] - Qs64[None, :, :]
            adq = np.abs(Qs64)[:, None, :] + np.abs(Qs64)[None, :, :]
            kq64 = sf264 * np.exp(-0.5 * (dq64 * dq64).sum(axis=2))
            ekq = EXP_ULPS + (np.abs(dq64) * (np.abs(dq64) + adq)).sum(axis=2) + 0.5 * D * (dq64 * dq64).sum(axis=2)
            eye = np.eye(M)
            res["cov"] = (kq + hp.arr(o["noise"][b] * eye) - V.T @ V, kq64 + o["noise"][b] * eye + Va.T @ Va,
                          kq64 * ekq * (1.0 - eye) + VE.T @ Va + Va.T @ VE)
        if "dvar" in outs:
            C, Ca, CE = W.T @ V, Wa.T @ Va, Wa.T @ VE          # (N, M)
            val = hp.zeros((M, D))
            sc, es = np.zeros((M, D)), np.zeros((M, D))
            for d in range(D):
                val[:, d] = (hp.arr(-2.0) / ls[d]) * (K * -df[:, :, d] * C.T).sum(axis=1)
                sc[:, d] = (2.0 / ls64[d]) * (K64 * ad[:, :, d] * Ca.T).sum(axis=1)
                es[:, d] = (2.0 / ls64[d]) * ((KE64 * Ca.T + K64 * CE.T) * ad[:, :, d]).sum(axis=1)
            res["dvar"] = (val, sc, es)
    return res


_refs = {}


def small_reference(c, ops=None, hp=None, keep=None):
    """{output: (value fp64-rounded from the reference's format, the value in that format, scale, escale)}, the B models' blocks
    stacked in the entry's layout: mean (B, M, P) ... ; "_raw" (B, M): kss - |W k*|^2 before the clip.  Cached per case."""
    cached = hp is None and keep is None and ops is None
    if cached and c in _refs:
        return _refs[c]
    ops = case_operands(c) if ops is None else ops
    hp = default_hp() if hp is None else hp
    outs = outputs_of(c)
    per = [_model_reference(hp, c, ops, b, outs, None if keep is None else keep[b]) for b in range(c.B)]
    res = {}
    for k in list(outs) + (["_raw"] if "var" in outs else []):
        if k == "_raw":
            res[k] = np.stack([p[k] for p in per])
            continue
        val = np.stack([p[k][0] for p in per])
        res[k] = (np.stack([hp.f64(p[k][0]) for p in per]), val, np.stack([p[k][1] for p in per]), np.stack([p[k][2] for p in per]))
    if cached:
        _refs[c] = res
    return res


def case_bars(c, ref=None):
    """{output: bar array}: 2^-53 (chain scale + escale), chains from the mirror at the case's largest chunk of queries."""
    ref = small_reference(c) if ref is None else ref
    chains = small_form(call_of(c), c.N, c.D, c.P, min(c.M, SQ), c.B).chains
    return {k: U * (chains[k] * ref[k][2] + ref[k][3]) for k in outputs_of(c)}


def error_ratio(hp, got64, ref_entry, bar):
    """max |got - reference| / bar, the difference taken in the reference's format."""
    return float(np.max(ratio(hp.f64(np.abs(hp.arr(got64) - ref_entry[1])), bar)))


def ratio(diff, bar):
    """diff / bar; where the bar is 0 (the far query's kernel row: every summand is 0) 0 for an exact result, else infinity."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bar > 0, diff / bar, np.where(diff == 0, 0.0, np.inf))


# ---- the same formulas in plain fp64 NumPy, in a chosen order ----------------------------------------------------------
def fp64_outputs(c, o, variant=0, keep=None):
    """Every output of the case's entry in fp64: variant 0 in NumPy's own order, 1 with the training rows reversed, 2 with a
    seeded permutation of the rows and the features summed backwards.  keep: per model a 0 / 1 weight per training row."""
    N, D, P, M = c.N, c.D, c.P, c.M
    outs = outputs_of(c)
    res = {k: [] for k in outs}
    perm = {0: np.arange(N), 1: np.arange(N)[::-1], 2: np.random.default_rng(7).permutation(N)}[variant]
    order = (lambda n: range(n - 1, -1, -1)) if variant == 2 else None
    for b in range(c.B):
        K, df, _, Qs = _kstar64(o, b, None if keep is None else keep[b], order)
        K, df = np.ascontiguousarray(K[:, perm]), np.ascontiguousarray(df[:, perm])
        alpha, ls, ys = o["alpha"][b][perm], o["ls"][b], o["ys"][b * P:(b + 1) * P]
        S = K @ alpha
        res["mean"].append(o["ym"][b * P:(b + 1) * P] + ys * S)
        if "dmean" in outs:
            res["dmean"].append(np.stack([(ys / ls[d]) * ((K * -df[:, :, d]) @ alpha) for d in range(D)], axis=2))
        if "hess" in outs:
            h = np.zeros((M, P, D, D))
            for d in range(D):
                for e in range(d + 1):
                    t = (K * df[:, :, d] * df[:, :, e]) @ alpha
                    h[:, :, d, e] = h[:, :, e, d] = ys / (ls[d] * ls[e]) * (t - S if d == e else t)
            res["hess"].append(h)
        if "var" in outs or "cov" in outs:
            W = np.ascontiguousarray(o["W"][b][:, :N][:, perm])
            V = W @ K.T
            if "var" in outs:
                res["var"].append(np.maximum(o["kss"][b] - (V * V).sum(axis=0), o["floor"]))
            if "cov" in outs:
                dq = Qs[:, None, :] - Qs[None, :, :]
                res["cov"].append(o["sf2"][b] * np.exp(-0.5 * (dq * dq).sum(axis=2)) + o["noise"][b] * np.eye(M) - V.T @ V)
            if "dvar" in outs:
                C = W.T @ V
                res["dvar"].append(np.stack([(-2.0 / ls[d]) * (K * -df[:, :, d] * C.T).sum(axis=1) for d in range(D)], axis=1))
    return {k: np.stack(v) for k, v in res.items()}


# ---- host tests --------------------------------------------------------------------------------------------------------
def test_long_double_is_extended_or_mpmath_takes_over():
    hp = default_hp()
    assert hp.kind == "mpmath" or np.finfo(np.longdouble).eps <= 2.0 ** -63
    one = hp.arr(1.0) + hp.arr(2.0 ** -62)
    assert hp.f64((one - hp.arr(1.0)) * hp.arr(2.0 ** 62)) == 1.0      # 63 bits are kept


def test_mirror_at_the_switch_points():
    f = small_form
    # NMB at M = 16 | 17
    assert (f("predict", 100, 9, 1, 16).nmb, f("predict", 100, 9, 1, 17).nmb) == (1, 2)
    # chunks per row block: Np = 128: 2 chunks and 6 idle waves; 640: 10, one pipelined round; 1152: 18, two rounds (wave 0: 0, 8, 16)
    assert [(x.nch, x.idle_waves, x.v_rounds) for x in (f("predict", n, 9, 1, 1) for n in (128, 640, 1152, 2100))] == \
        [(2, 6, 1), (10, 0, 1), (18, 0, 2), (34, 0, 3)]
    # the variance's shares: gb = 8 for 16 parts; 136 = 8.5 per part: a second round of eight
    assert [(x.gb, x.var_share_rounds) for x in (f("predict", n, 9, 1, 1) for n in (128, 2048, 2100))] == [(8, 1), (128, 1), (136, 2)]
    # finish_means: 4, 2, 1 parts at M P = 64 | 65, 128 | 135, and two passes from 257
    assert [(f("predict", 100, 9, p, m).fm_parts, f("predict", 100, 9, p, m).fm_passes)
            for m, p in ((1, 1), (4, 16), (5, 13), (8, 16), (9, 15), (16, 16), (17, 16), (32, 16))] == \
        [(4, 1), (4, 1), (2, 1), (2, 1), (1, 1), (1, 1), (1, 2), (1, 2)]
    # finish_jac: passes of 4 x 256 entries
    assert [f("grad", 100, d, p, m).fj_passes for m, p, d in ((1, 1, 1), (32, 2, 16), (5, 13, 16), (32, 16, 16))] == [1, 1, 2, 8]
    # covariance: groups of 16 workgroups, the top level in rounds of 8
    assert [(x.gb, x.cov_groups, x.cov_top_rounds) for x in (f("cov", n, 9, 1, 1) for n in (128, 256, 384, 2176))] == \
        [(8, 1, 1), (16, 1, 1), (24, 2, 1), (136, 9, 2)]
    # row chunks of the W^T V launch, and the final sum's passes of 256 entries
    assert [f("grad", n, 9, 1, 1, b).rc for n, b in ((128, 1), (1024, 1), (2048, 1), (2176, 1), (256, 8), (512, 8), (128, 8))] == [4, 4, 2, 1, 2, 1, 4]
    assert (f("grad", 100, 16, 1, 32).wtv_passes, f("grad", 100, 16, 1, 16).wtv_passes) == (2, 1)
    # Hessian: rows, rounds of 32, groups; slices
    assert [(x.hess_rows, x.hess_rounds, x.hess_groups) for x in (f("hess", n, 9, 1, 1) for n in (1, 2048, 2176, 3072, 4096, 16384))] == \
        [(32, 1, 4), (32, 1, 64), (34, 2, 64), (48, 2, 64), (64, 2, 64), (256, 8, 64)]
    assert [(hess_slice(d), f("hess", 100, d, p, m).slices) for m, p, d in ((32, 16, 1), (32, 2, 16), (25, 6, 10), (1, 1, 9))] == \
        [(256, 2), (3, 22), (9, 17), (11, 1)]
    # chains, counted by hand at N = 1000, M = 1, P = 1: ga 32, gb 64, 16 chunks -> 2 per wave
    ch = f("grad", 1000, 9, 1, 1).chains
    assert ch["mean"] == 1 + 32 + 8 + 3 + 2 and ch["var"] == 2 * (1 + 128 + 8) + 1 + 16 + 4 + 16 + 1
    assert ch["cov"] == 2 * 137 + 16 + 16 + 4 + 2 and ch["dmean"] == 5 + 32 + 32 + 2
    assert ch["dvar"] == (137 + 16 + 16) + 4 + 16 + 128 + 1 + 2 and ch["hess"] == 8 + 32 + 32 + 1 + 3
    assert form_words(GROUPS["D"][7]) == ["grad", "1", "1", "2176", "17", "9", "3", "ga68", "gb136", "nmb2", "rc1", "hg0", "sl0"]
    assert case_lines(GROUPS["A"][8]) == [["predict", "1", "1", "256", "32", "9", "16", "ga8", "gb16", "nmb0", "rc0", "hg0", "sl0"],
                                          ["predict", "1", "1", "256", "1", "9", "16", "ga8", "gb16", "nmb0", "rc0", "hg0", "sl0"]]


def test_every_switch_point_is_a_case():
    forms = {c: small_form(call_of(c), c.N, c.D, c.P, min(c.M, SQ), c.B) for c in ALL_CASES}
    var = [f for c, f in forms.items() if "var" in outputs_of(c)]
    assert {1, 2} <= {f.nmb for f in var} and {1, 2, 3} <= {f.v_rounds for f in var} and any(f.idle_waves for f in var)
    assert {1, 2} <= {f.var_share_rounds for f in var}
    assert {(4, 1), (2, 1), (1, 1), (1, 2)} <= {(f.fm_parts, f.fm_passes) for f in forms.values()}
    assert {1, 2, 8} <= {f.fj_passes for c, f in forms.items() if c.entry == "grad"}
    assert {(8, 1), (16, 1), (24, 2), (136, 9)} <= {(f.gb, f.cov_groups) for c, f in forms.items() if call_of(c) == "cov"}
    assert {1, 2, 4} <= {f.rc for f in forms.values()} and {1, 2} <= {f.wtv_passes for f in forms.values()}
    assert {(32, 4), (34, 64), (64, 64)} <= {(f.hess_rows, f.hess_groups) for c, f in forms.items() if call_of(c) == "hess"}
    assert {1, 2, 17, 22} <= {f.slices for f in forms.values()}
    assert {2, 8} == {c.B for c in GROUPS["F"]} and all(padded(c.N) <= 4096 for c in ALL_CASES)
    assert any(c.N == padded(c.N) for c in GROUPS["B"]) and any(c.N == padded(c.N) - 127 for c in GROUPS["B"])
    assert [call_of(c) for c in SEQUENCE] == ["cov", "hess", "grad", "cov", "predict", "predict"] and SEQUENCE[0].B == 8


@pytest.mark.parametrize("c", ALL_CASES, ids=case_id)
def test_operands_are_what_the_docstring_says(c):
    o = case_operands(c)
    Np = padded(c.N)
    for b in range(c.B):
        W = o["W"][b]
        assert W.shape == (Np, Np) and not np.triu(W, 1).any() and (W.diagonal() > 0).all() and (np.tril(W, -1) != 0).mean() > 0.49
        assert (o["ls"][b] >= 0.7 * math.sqrt(c.D)).all() and (o["ls"][b] <= 2.5 * math.sqrt(c.D)).all()
        assert (np.abs(o["alpha"][b]) >= 0.5).all() and (c.N < 8 or ((o["alpha"][b] < 0).any() and (o["alpha"][b] > 0).any()))
        K = _kstar64(o, b)[0]
        if c.M >= 5:
            assert not K[c.M - 1].any(), "the far query's kernel row is exactly zero"
            assert (K[:c.M - 1] > 0).all()
    if c.M >= 4:
        assert np.array_equal(o["Xq"][2], o["Xq"][3]) and np.array_equal(o["Xq"][0], o["X"][0][0]) and np.array_equal(o["Xq"][1], o["X"][0][c.N - 1])
    ref = small_reference(c)
    if c.M >= 5:
        P = c.P
        assert np.array_equal(ref["mean"][0][:, c.M - 1, :].reshape(-1), o["ym"][:c.B * P])
        if "var" in ref and c.regime != "clip":
            assert np.array_equal(ref["var"][0][:, c.M - 1], np.array(o["kss"]))
    if c.regime == "clip":
        clipped = ref["_raw"] < o["floor"]
        assert 8 <= clipped.sum() <= c.M - 8 and np.array_equal(ref["var"][0][clipped], np.full(int(clipped.sum()), o["floor"]))
        assert (np.abs(ref["_raw"] - o["floor"]) > 1e3 * case_bars(c)["var"]).all(), "no variance sits at the clip"


@pytest.mark.parametrize("c", ALL_CASES, ids=case_id)
def test_fp64_numpy_in_any_order_stays_within_the_bars(c):
    hp, o, ref, bars = default_hp(), case_operands(c), small_reference(c), case_bars(c)
    worst = 0.0
    for variant in range(3):
        got = fp64_outputs(c, o, variant)
        for k in outputs_of(c):
            r = error_ratio(hp, got[k], ref[k], bars[k])
            worst = max(worst, r)
            assert r <= 1.0, (k, variant, r)
    print(f"{case_id(c)}: fp64 NumPy, three orders: largest error / bar {worst:.3f}")


@pytest.mark.parametrize("c", ALL_CASES, ids=case_id)
def test_one_lost_block_of_32_rows_leaves_the_bars(c):
    """Any 32 training rows dropped from K* (every block up to 8, else the first, the last and six seeded ones) move every output
    by at least 100 bars somewhere (fp64 differences: a sensitivity, not an accuracy)."""
    o, bars = case_operands(c), case_bars(c)
    full = fp64_outputs(c, o)
    nb = _ceil(c.N, 32)
    blocks = range(nb) if nb <= 8 else sorted({0, nb - 1, *np.random.default_rng(3).choice(nb, 6, replace=False).tolist()})
    least = math.inf
    for blk in blocks:
        keep = np.ones(c.N)
        keep[32 * blk:32 * blk + 32] = 0.0
        got = fp64_outputs(c, o, keep=[keep] * c.B)
        for k in outputs_of(c):
            r = float(np.max(ratio(np.abs(got[k] - full[k]), bars[k])))
            least = min(least, r)
            assert r >= 100.0, (k, blk, r)
    print(f"{case_id(c)}: a lost block of 32 rows: at least {least:.2e} bars")


def test_true_inverse_factor_gives_the_closed_form_posterior():
    c = _c("X", "grad_var", 100, 3, 2, 6)
    o = {k: (list(v) if isinstance(v, list) else v) for k, v in case_operands(c).items()}
    X, ls, sf2, noise = o["X"][0], o["ls"][0], o["sf2"][0], o["noise"][0]
    Xs = X / ls
    Kxx = sf2 * np.exp(-0.5 * ((Xs[:, None, :] - Xs[None, :, :]) ** 2).sum(axis=2)) + noise * np.eye(c.N)
    Y = np.random.default_rng(5).standard_normal((c.N, c.P))
    Np = padded(c.N)
    W = np.eye(Np)
    W[:c.N, :c.N] = np.linalg.inv(np.linalg.cholesky(Kxx))
    Kinv = np.linalg.inv(Kxx)
    o["W"], o["alpha"], o["kss"] = [W], [Kinv @ Y], [sf2 + noise]
    ref = small_reference(c, ops=o)
    Ks = _kstar64(o, 0)[0]
    assert np.allclose(ref["mean"][0][0], o["ym"] + o["ys"] * (Ks @ Kinv @ Y), rtol=1e-9, atol=1e-9)
    assert np.allclose(ref["var"][0][0], np.maximum(sf2 + noise - np.einsum("mj,jk,mk->m", Ks, Kinv, Ks), FLOOR), rtol=1e-8, atol=1e-10)
    cc = Case("X", "cov", c.N, c.D, c.P, c.M, 1, 0, "plain")
    Qs = o["Xq"] / ls
    Kqq = sf2 * np.exp(-0.5 * ((Qs[:, None, :] - Qs[None, :, :]) ** 2).sum(axis=2)) + noise * np.eye(c.M)
    assert np.allclose(small_reference(cc, ops=o)["cov"][0][0], Kqq - Ks @ Kinv @ Ks.T, rtol=1e-8, atol=1e-10)
    # the gradients against central differences of the closed form
    h = 1e-5
    for d in range(c.D):
        op, om = dict(o), dict(o)
        e = np.zeros(c.D)
        e[d] = h
        op["Xq"], om["Xq"] = o["Xq"] + e, o["Xq"] - e
        Kp, Km = _kstar64(op, 0)[0], _kstar64(om, 0)[0]
        dm = o["ys"] * ((Kp - Km) @ Kinv @ Y) / (2 * h)
        dv = -(np.einsum("mj,jk,mk->m", Kp, Kinv, Kp) - np.einsum("mj,jk,mk->m", Km, Kinv, Km)) / (2 * h)
        assert np.allclose(ref["dmean"][0][0][:, :, d], dm, rtol=1e-5, atol=1e-7)
        assert np.allclose(ref["dvar"][0][0][:, d], dv, rtol=1e-5, atol=1e-7)
    ch = Case("X", "hess", c.N, c.D, c.P, c.M, 1, 0, "plain")
    hs = small_reference(ch, ops=o)["hess"][0][0]
    for d in range(c.D):
        op, om = dict(o), dict(o)
        e = np.zeros(c.D)
        e[d] = h
        op["Xq"], om["Xq"] = o["Xq"] + e, o["Xq"] - e
        jp = small_reference(Case("X", "grad", c.N, c.D, c.P, c.M, 1, 0, "plain"), ops=op)["dmean"][0][0]
        jm = small_reference(Case("X", "grad", c.N, c.D, c.P, c.M, 1, 0, "plain"), ops=om)["dmean"][0][0]
        assert np.allclose(hs[:, :, :, d], (jp - jm) / (2 * h), rtol=1e-5, atol=1e-7)


def test_mpmath_path_agrees_with_long_double():
    c = _c("X", "grad_var", 40, 3, 2, 5)
    a = small_reference(c, hp=HP("mpmath"))
    cc = Case("X", "cov", 40, 3, 2, 5, 1, 0, "plain")
    ch = Case("X", "hess", 40, 3, 2, 5, 1, 0, "plain")
    a.update({k: v for k, v in small_reference(cc, ops=case_operands(c), hp=HP("mpmath")).items() if k == "cov"})
    a.update({k: v for k, v in small_reference(ch, ops=case_operands(c), hp=HP("mpmath")).items() if k == "hess"})
    if np.finfo(np.longdouble).eps > 2.0 ** -63:
        return
    b = small_reference(c, hp=HP("longdouble"))
    b.update({k: v for k, v in small_reference(cc, ops=case_operands(c), hp=HP("longdouble")).items() if k == "cov"})
    b.update({k: v for k, v in small_reference(ch, ops=case_operands(c), hp=HP("longdouble")).items() if k == "hess"})
    for k in ("mean", "var", "dmean", "dvar", "cov", "hess"):
        assert np.max(ratio(np.abs(a[k][0] - b[k][0]), a[k][2])) <= 2.0 ** -52, k
        assert np.array_equal(a[k][2], b[k][2])
