"""The references, the launch-rule restatement, the emulations and the bars of tests/test_gpu_mean_mfma_forms.py (the matrix-core
posterior mean of gpk_mean.hip: mean_prep_kernel, mean_bf16_kernel for D <= 14, mean_mfma_kernel<9> for D = 15, 16 and
mean_mfma_reduce_kernel), checked here without a GPU:

* `mean_mfma_form`: the launch rule of gpk_predict_mean_mfma - QB, nqb, S, chunk, the 32-point blocks of every chunk, the size of
  the last block, the staging rounds of the fp32-MFMA kernel - asserted at the sizes where the form changes;
* `case_operands`: X, Xq fp32 standard normal rows, ls = 0.7 sqrt(D) (1 + 0.02 d), sf2 = 1.3, y_mean = +-0.25 (p + 1),
  y_std = 0.6 + 0.15 p, and one of three regimes:
  "share":  alpha uniform in [0.5, 1.5], centre = the training mean.  Nothing cancels: every query's sum s_mp = sum_j k_mj alpha_jp is
            positive and differs across queries and outputs.  Asserted for every GPU case: every whole 32-point block carries at
            least 1 / (4 nblk) of every query's sum, and for M >= 64 every training point has a query in which its share exceeds
            8 bar;
  "gate":   the centre moved off the training mean along the diagonal of the scaled coordinates until 48 <= |u|^2 <= 64 holds for
            every training and query point (u = sqrt(log2(e) / 2) (x - centre) / ls as the kernel forms it, in fp32): the edge of what
            device.py admits (MFMA_MEAN_R2_MAX).  "gate0" is the same data with the centre at the training mean;
  "signed": alpha with random signs; the error is measured against sqrt(sum_j (k_mj alpha_jp)^2).  "signed0": the queries are
            training rows (d = 0 on the diagonal).
* `mean_reference`: the mean in fp64 from the fp32 operands with exact differences (`rbf_panel`), sf2, y_mean, y_std in fp64;
* `emu_distances`, `emu_accumulate`: NumPy emulations of both kernels' arithmetic - centred, scaled fp32 coordinates, |u|^2 by an
  fp32 FMA chain; D <= 14: the exact three-way bf16 split and the six products in chain6's order, each summed exactly and rounded
  to fp32 once; D = 15, 16: nine fp32 steps of two components each from the |u_q|^2 seed; exp2 in fp32; the per-lane fp32 running
  sums over the blocks of a chunk in order, the lane butterfly in the kernel's mask order (16 .. 1 for bf16, 1 .. 16 for fp32-MFMA),
  the fp64 sum over chunks and the reduce kernel's fp32 epilogue - complete, and with one of a1 b0, a0 b1, a1 b1, a0 b2, a2 b0 left
  out;
* the bar of a case, from the reference side only: e = the largest error over queries and outputs relative to y_std sf2 s ("share",
  "gate") or y_std sf2 sqrt(sum (k alpha)^2) ("signed"); bar = 4 e_full (the complete emulation's e; the 4 covers v_exp_f32's
  rounding and the matrix pipe's internal summation); a gate case claims a second-order product where the emulation without it
  errs by at least 8 e_full, and its bar is then at most a quarter of that error.  Asserted for every GPU case: each planted
  fault moves the reference by more than 4 bar - one 32-point block dropped for one 32-query block (first, last, interior), point 0
  dropped, the last live point dropped, two query rows of one block exchanged, outputs p and p + 1 exchanged - and so does each
  first-order product left out (bf16 cases).  Cases of more than 2048 queries: everything here on the first 128 and last 256.

Four things about the operands are not what one would first write down:
* the ragged last block (8 points at N = 200, 1 at N = 513, 4 at N = 4100) cannot carry 1 / (4 nblk) of a sum of equal-sized terms
  for EVERY query - a single point is near some queries and far from others - so the share floor is asked of the whole blocks.
  Dropping the last block, ragged or not, is one of the planted faults and must move e by more than 4 bar like the others;
* with one feature (D = 1) a block of 32 standard normal points can miss the neighbourhood of an outlying query altogether: of
  eight draws tried (alpha = 1), four kept every block above the floor at D = 1, and the seeds here are one of those.  Every other
  (N, M, D) held it in all eight;
* with standard normal rows and these length-scales the cloud of u is about 4 across and the shell 48 <= |u|^2 <= 64 is 1.07 thick:
  no centre puts every point inside.  The gate cases contract the same kind of rows by 1 / 4 (exact in fp32) before the centre is
  moved; the asserted bound is unchanged.  |u|^2 then spans 51.8 .. 60.2 (D = 9) to 53.1 .. 58.9 (D = 16), and 0.01 .. 0.23 centred.
* N = 1: the single point is the centre, b = (0, .., 0, 1) and its parts b1 = b2 = 0: a0 b1, a1 b1, a0 b2 change no bit and no bar is
  asked to stay under them (asserted: these three, only at N = 1).

Measured here, per case group (e_full / without a1 b0 / a0 b1 / a1 b1 / a0 b2 / a2 b0 / the smallest planted fault / bar; every case
prints its own):
A  bf16, P 1 .. 8:      4.3e-7 .. 5.2e-7 / 5.3e-3 / 4.1e-4 .. 5.5e-4 / 4.7e-7 .. 7.0e-7 / 4.8e-7 .. 5.8e-7 / 9.6e-6 .. 9.8e-6 / 1.6e-2 / 1.7e-6 .. 2.1e-6
B  bf16, D 1 .. 14:     3.3e-7 .. 6.6e-7 / 4.7e-3 .. 2.6e-2 / 2.9e-4 .. 5.1e-3 / 5.4e-7 .. 1.0e-5 / 6.2e-7 .. 1.6e-5 / 6.6e-6 .. 4.3e-5 / 1.5e-2 / 1.3e-6 .. 2.6e-6
C  bf16, edges:         8.2e-8 (M = 1) .. 1.4e-5 (N = 1) / 2.8e-3 .. 2.1e-2 / 8.4e-5 .. 1.6e-3 (N > 1) / 8.2e-8 .. 1.4e-5 / 1.0e-7 .. 1.4e-5 /
                        2.6e-7 .. 3.3e-5 / 6.4e-4 (point 0 of 4100) / 3.3e-7 .. 5.5e-5; every fault at least 390 bar
D  fp32-MFMA:           2.6e-7 .. 9.8e-7 (N = 1) / - / 3.4e-4 (point 0 of 4100) / 1.0e-6 .. 3.9e-6; every fault at least 217 bar
E  gate, bf16:          5.6e-6 .. 6.7e-6 / 0.18 .. 0.22 / 1.0e-3 .. 1.4e-3 / 1.1e-5 .. 1.2e-5 / 8.5e-6 .. 1.1e-5 / 2.3e-4 .. 2.9e-4 / 2.3e-3 / 2.2e-5 .. 2.7e-5
   gate, fp32-MFMA:     6.3e-6 .. 6.7e-6 / - / 2.2e-3 / 2.5e-5 .. 2.7e-5
   centred, bf16:       1.9e-7 .. 2.4e-7 / 3.2e-4 .. 3.4e-4 / 8.8e-6 .. 1.0e-5 / 2.0e-7 .. 2.4e-7 / 1.9e-7 .. 2.4e-7 / 6.2e-7 .. 7.6e-7 / 2.3e-3 / 7.6e-7 .. 9.5e-7
   centred, fp32-MFMA:  2.1e-7 .. 2.2e-7 / - / 2.2e-3 / 8.5e-7 .. 8.9e-7
F  signed, bf16:        5.7e-7 .. 6.1e-7 / 9.3e-3 .. 9.8e-3 / 6.2e-3 .. 6.4e-3 / 5.5e-6 .. 1.4e-5 / 8.0e-6 .. 9.1e-6 / 1.2e-5 .. 1.9e-5 / 0.12 / 2.3e-6 .. 2.5e-6
   signed, fp32-MFMA:   5.2e-7 / - / 0.11 / 2.1e-6
G  bf16 / fp32-MFMA:    3.4e-7 / 5.4e-3 / 8.4e-5 / 3.3e-7 / 3.9e-7 / 1.1e-5 / 2.0e-3 / 1.4e-6   and   3.9e-7 / - / 1.2e-3 / 1.5e-6
Share regime: the smallest whole-block share is 0.33 / nblk (D = 1), 0.48 / nblk and more elsewhere; every point's best share is at
least 116 bar.  The second-order products at the gate, against the prediction that all three show there: without a2 b0 the
emulation errs by 34 .. 51 e_full - the lost part of |u_q|^2 (2^-18 x 56) is the same for every training point and shifts the whole
sum - and every bf16 gate case claims it; without a0 b2 or a1 b1 it errs by 1.5 .. 1.9 e_full only - those parts differ from point to
point and average out over the 600 terms - and no case claims them.  Centred, none of the three reaches 4 e_full.  (Away from the
gate a2 b0 still moves the share cases by about 1e-5, 20 e_full; only the gate cases lower their bar for it.)

NumPy and torch (CPU) only."""
import collections
import functools

import numpy as np
import pytest

from test_gram_refs import rbf_panel
from test_k5_refs import split3_parts

SF2 = 1.3
S_CONST = 0.84932180028801904          # sqrt(log2(e) / 2), as gpk_predict_mean_mfma has it
MM_TJ = 512
EMU_MAX_M, EMU_HEAD, EMU_TAIL = 2048, 128, 256
GATE_SHRINK = 0.25
CHAIN6 = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
FIRST_ORDER, SECOND_ORDER = ("a1b0", "a0b1"), ("a1b1", "a0b2", "a2b0")
f32, f64 = np.float32, np.float64


# ---- the launch rule --------------------------------------------------------------------------------------------------
Form = collections.namedtuple("Form", "kernel QB nqb S chunk nb last rounds")


def mean_mfma_form(N, M, D, P):
    """gpk_predict_mean_mfma's launch: kernel "bf16" (D <= 14) or "f32", QB query blocks of 32 per wave, nqb workgroups of 128 QB
    queries, S chunks of `chunk` training points (a multiple of 512), nb[s] = the 32-point blocks of chunk s, last = the points of
    the last block, rounds[s] = the points of every 512-point staging round of chunk s (the fp32-MFMA kernel)."""
    QB = 2 if P <= 3 else 1
    nqb = -(-M // (128 * QB))
    S = -(-1024 // nqb)
    S = max(S, -(-N // 2048))
    S = max(1, min(S, -(-N // MM_TJ), 65535))
    chunk = -(-(-(-N // S)) // MM_TJ) * MM_TJ
    S = -(-N // chunk)
    ends = [min(N, (s + 1) * chunk) - s * chunk for s in range(S)]
    nb = tuple(-(-n // 32) for n in ends)
    rounds = tuple(tuple(min(MM_TJ, n - r) for r in range(0, n, MM_TJ)) for n in ends)
    return Form("bf16" if D <= 14 else "f32", QB, nqb, S, chunk, nb, N - (N - 1) // 32 * 32, rounds)


def form_words(N, M, D, P):
    """The words of the library's GPKMEANMM line for this call."""
    f = mean_mfma_form(N, M, D, P)
    return [f.kernel, str(N), str(M), str(D), str(P), f"qb{f.QB}", f"nqb{f.nqb}", f"s{f.S}", f"chunk{f.chunk}"]


# ---- the cases of the GPU module --------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "regime N M D P")
BIG3, BIG4 = 262144 + 5, 131072 + 5
GROUPS = {
    "A": [Case("share", 200, 300, 9, P) for P in range(1, 9)],
    "B": [Case("share", 200, 300, D, P) for D in (1, 6, 7, 8, 13, 14) for P in (3, 5)],
    "C": [Case("share", N, 300, 9, P) for N in (1, 20, 32, 33, 64, 513, 544, 608, 2144) for P in (3, 4)]
         + [Case("share", 200, M, 9, P) for M in (1, 255, 256, 257) for P in (3, 4)]
         + [Case("share", 2048, BIG3, 9, 3), Case("share", 2048, BIG4, 9, 4), Case("share", 4100, 90000, 9, 3), Case("share", 4100, 90000, 9, 4)],
    "D": [Case("share", 200, 300, D, P) for D in (15, 16) for P in range(1, 9)]
         + [Case("share", N, 300, 16, 3) for N in (1, 33, 513)] + [Case("share", 1024, 262144, 16, 3), Case("share", 4100, 90000, 16, 3)],
    "E": [Case("gate", 600, 300, D, P) for D in (9, 14) for P in (3, 6)] + [Case("gate", 600, 300, D, 3) for D in (15, 16)],
    "F": [Case("signed", 600, 300, 9, 3), Case("signed", 600, 300, 16, 3), Case("signed0", 600, 300, 9, 5)],
    "G": [Case("share", 2144, 300, 9, 3), Case("share", 2600, 300, 16, 5)],
}
GATE0 = [c._replace(regime="gate0") for c in GROUPS["E"]]


def case_id(c):
    return f"{c.regime}-N{c.N}-M{c.M}-D{c.D}-P{c.P}"


ALL_CASES = list(dict.fromkeys(c for g in GROUPS.values() for c in g)) + GATE0


# ---- the operands -----------------------------------------------------------------------------------------------------
def ls_of(D):
    return 0.7 * np.sqrt(D) * (1.0 + 0.02 * np.arange(D))


def scaled(x32, ls, center):
    """u as both kernels form it: (x - fp32(centre)) * fp32(sqrt(log2(e) / 2) / ls), two fp32 roundings."""
    return (x32 - np.asarray(center, dtype=f64).astype(f32)) * (S_CONST / np.asarray(ls, dtype=f64)).astype(f32)


def fma32(a, b, c):
    return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


def norm2(u):
    """|u|^2 by the kernels' fp32 FMA chain over the features in order."""
    s = np.zeros(u.shape[0], dtype=f32)
    for d in range(u.shape[1]):
        s = fma32(u[:, d], u[:, d], s)
    return s


def _gate_center(X, Xq, ls):
    """The training mean moved along the diagonal of the scaled coordinates until the |u|^2 of all points straddle 56 evenly."""
    mean = X.astype(f64).mean(axis=0)
    both = np.concatenate([X, Xq])
    lo, hi = 0.0, 16.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        r2 = norm2(scaled(both, ls, mean + mid / np.sqrt(len(ls)) * ls / S_CONST)).astype(f64)
        lo, hi = (mid, hi) if 0.5 * (r2.min() + r2.max()) < 56.0 else (lo, mid)
    return mean + lo / np.sqrt(len(ls)) * ls / S_CONST


@functools.lru_cache(maxsize=None)
def case_operands(c):
    """dict(X (N, D) fp32, Xq (M, D) fp32, alpha (N, P) fp32, ls, center, ym, ys) of a case; arrays are read-only."""
    N, M, D, P = c.N, c.M, c.D, c.P
    X = np.random.default_rng(63000 + 7 * N + 16 * D).standard_normal((N, D)).astype(f32)
    Xq = np.random.default_rng(64000 + 7 * M + 16 * D).standard_normal((M, D)).astype(f32)
    alpha = (0.5 + np.random.default_rng(66000 + 7 * N + P).random((N, P))).astype(f32)
    ls = ls_of(D)
    if c.regime in ("gate", "gate0"):
        X, Xq = X * f32(GATE_SHRINK), Xq * f32(GATE_SHRINK)
    if c.regime in ("signed", "signed0"):
        alpha *= np.random.default_rng(67000 + N + P).choice(np.array([-1.0, 1.0], dtype=f32), size=(N, P))
    if c.regime == "signed0":
        Xq = X[np.random.default_rng(68000 + M).permutation(N)[:M]].copy()
    center = _gate_center(X, Xq, ls) if c.regime == "gate" else X.astype(f64).mean(axis=0)
    ym = 0.25 * (np.arange(P) + 1.0) * np.where(np.arange(P) % 2 == 0, 1.0, -1.0)
    ys = 0.6 + 0.15 * np.arange(P)
    for a in (X, Xq, alpha):
        a.setflags(write=False)
    return dict(X=X, Xq=Xq, alpha=alpha, ls=ls, center=center, ym=ym, ys=ys)


def emu_rows(M):
    """The queries the emulations and the CPU-side assertions run on."""
    return np.arange(M) if M <= EMU_MAX_M else np.concatenate([np.arange(EMU_HEAD), np.arange(M - EMU_TAIL, M)])


# ---- the reference ----------------------------------------------------------------------------------------------------
def mean_reference(ops, Xq, signed, device=None):
    """(mean, den) as fp64 torch tensors (m, P): mean = y_mean + y_std sf2 sum_j k_mj alpha_jp with k from `rbf_panel` of the fp32
    operands; den = what the error is measured against: y_std sf2 s, or y_std sf2 sqrt(sum_j (k_mj alpha_jp)^2) where `signed`."""
    import torch
    t = lambda a: a.to(device, torch.float64) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=f64), device=device)      # noqa: E731
    K = rbf_panel(t(Xq), np.asarray(ops["X"], dtype=f64), ops["ls"], 1.0)
    al = t(ops["alpha"])
    s = K @ al
    den = torch.sqrt((K * K) @ (al * al)) if signed else s.abs()
    return t(ops["ym"]) + t(ops["ys"]) * SF2 * s, t(ops["ys"]) * SF2 * den


def rel_err(got, ref, den):
    return float(np.max(np.abs(np.asarray(got, dtype=f64) - ref) / den))


# ---- the emulations ---------------------------------------------------------------------------------------------------
def emu_distances(ops, Xq, D, kernel):
    """The exponent d (m, N) fp32 of the complete product, and a function drop -> d without that product (bf16 only)."""
    u, uq = scaled(ops["X"], ops["ls"], ops["center"]), scaled(Xq, ops["ls"], ops["center"])
    tn, qn = norm2(u), norm2(uq)
    if kernel == "bf16":
        A, B = np.zeros((uq.shape[0], 16), dtype=f32), np.zeros((u.shape[0], 16), dtype=f32)
        A[:, :D], A[:, D], A[:, D + 1] = uq, 1.0, qn
        B[:, :D], B[:, D], B[:, D + 1] = f32(-2.0) * u, tn, 1.0
        a, b = [p.astype(f64) for p in split3_parts(A)], [p.astype(f64) for p in split3_parts(B)]
        prod = {(i, j): a[i] @ b[j].T for i, j in CHAIN6}       # bf16 x bf16 products and their sum of 16 are exact in fp64

        def chain(drop=None):
            c = np.zeros(prod[0, 0].shape, dtype=f32)
            for i, j in CHAIN6:
                if drop != f"a{i}b{j}":
                    c = (c.astype(f64) + prod[i, j]).astype(f32)
            return c
        return chain
    A, B = np.zeros((uq.shape[0], 18), dtype=f64), np.zeros((u.shape[0], 18), dtype=f64)
    A[:, :D], A[:, D] = uq, 1.0
    B[:, :D], B[:, D] = f32(-2.0) * u, tn

    def chain(drop=None):
        assert drop is None
        c = np.repeat(qn[:, None], u.shape[0], axis=1)
        for i in range(9):                                        # v_mfma_f32_32x32x2_f32: two components per step
            c = (c.astype(f64) + np.outer(A[:, 2 * i], B[:, 2 * i]) + np.outer(A[:, 2 * i + 1], B[:, 2 * i + 1])).astype(f32)
        return c
    return chain


def emu_accumulate(d32, ops, form):
    """mean (m, P) fp32 from the exponents: exp2 in fp32, per-lane running sums over the blocks of a chunk, the lane butterfly, the
    fp64 sum over chunks, the reduce kernel's epilogue."""
    alpha = ops["alpha"]
    N, P = alpha.shape
    e = np.exp2(-d32)
    assert e.dtype == f32
    total = np.zeros((e.shape[0], P), dtype=f64)
    for s in range(form.S):
        n0, n1 = s * form.chunk, min(N, (s + 1) * form.chunk)
        acc = np.zeros((e.shape[0], 32, P), dtype=f32)
        for j0 in range(n0, n1, 32):
            w = min(32, n1 - j0)
            acc[:, :w] = fma32(e[:, j0:j0 + w, None], alpha[None, j0:j0 + w, :], acc[:, :w])
        v = acc
        for step in range(5):
            h = v.shape[1] // 2
            v = v[:, :h] + v[:, h:] if form.kernel == "bf16" else v[:, 0::2] + v[:, 1::2]     # masks 16 .. 1 / 1 .. 16
        assert v.dtype == f32 and v.shape[1] == 1
        total += v[:, 0].astype(f64)
    return reduce_epilogue(total, ops)


def reduce_epilogue(total64, ops):
    """mean_mfma_reduce_kernel's last line in fp32: fp32(y_mean) + fp32(y_std) * (fp32(sf2) * fp32(s))."""
    return ops["ym"].astype(f32) + ops["ys"].astype(f32) * (f32(SF2) * total64.astype(f32))


# ---- bars and planted faults ------------------------------------------------------------------------------------------
def planted_faults(c, ops, rows, K, mean, den):
    """{name: the reference's movement} - max |mean' - mean| / den over the emulated rows - of the faults of the module docstring.
    K (m, N) fp64 NumPy: the kernel values of `rows`."""
    N, M, P = c.N, c.M, c.P
    al, scale = ops["alpha"].astype(f64), ops["ys"] * SF2
    nblk, out = -(-N // 32), {}
    qblocks = {"first": 0, "last": (M - 1) // 32, "interior": int(rows[len(rows) // 2]) // 32}
    pblocks = {"first": 0, "last": nblk - 1, "interior": nblk // 2}
    for where in ("first", "last", "interior"):
        r = np.nonzero(rows // 32 == qblocks[where])[0]
        j = slice(32 * pblocks[where], min(N, 32 * pblocks[where] + 32))
        out[f"block {where}"] = float(np.max(np.abs(scale * (K[r, j] @ al[j])) / den[r]))
    out["point 0"] = float(np.max(np.abs(scale * (K[:, :1] @ al[:1])) / den))
    out["last point"] = float(np.max(np.abs(scale * (K[:, N - 1:] @ al[N - 1:])) / den))
    if M >= 2:
        out["rows exchanged"] = float(np.max(np.abs(mean[0] - mean[1]) / np.minimum(den[0], den[1])))
    if P >= 2:
        out["outputs exchanged"] = min(float(np.max(np.abs(mean[:, p] - mean[:, p + 1]) / np.minimum(den[:, p], den[:, p + 1]))) for p in range(P - 1))
    return out


@functools.lru_cache(maxsize=None)
def case_figures(c):
    """Everything the reference side says about a case: dict(form, bar, e_full, drops {product: e}, claims (the second-order
    products the case claims to detect), faults {name: movement}, shares (min block share x nblk, min over points of the best
    share) for the share regime)."""
    import torch
    ops = case_operands(c)
    form = mean_mfma_form(c.N, c.M, c.D, c.P)
    rows = emu_rows(c.M)
    Xq = ops["Xq"][rows]
    signed = c.regime.startswith("signed")
    mean, den = (t.numpy() for t in mean_reference(ops, Xq, signed))
    chain = emu_distances(ops, Xq, c.D, form.kernel)
    e_full = rel_err(emu_accumulate(chain(), ops, form), mean, den)
    drops, inert = {}, ()
    if form.kernel == "bf16":
        full = chain()
        drops = {d: rel_err(emu_accumulate(chain(d), ops, form), mean, den) for d in FIRST_ORDER + SECOND_ORDER}
        inert = tuple(d for d in FIRST_ORDER + SECOND_ORDER if np.array_equal(chain(d), full))      # leaving it out changes no bit
    bar, claims = 4.0 * e_full, ()
    if c.regime == "gate" and drops:
        claims = tuple(d for d in SECOND_ORDER if drops[d] >= 8.0 * e_full)
        bar = min([bar] + [drops[d] / 4.0 for d in claims])
    K = rbf_panel(torch.as_tensor(Xq.astype(f64)), ops["X"].astype(f64), ops["ls"], 1.0).numpy()
    out = dict(form=form, bar=bar, e_full=e_full, drops=drops, claims=claims, inert=inert, faults=planted_faults(c, ops, rows, K, mean, den))
    if c.regime == "share":
        al = ops["alpha"].astype(f64)
        s = K @ al
        nblk = -(-c.N // 32)
        full = min(float(np.min((K[:, 32 * b:32 * b + 32] @ al[32 * b:32 * b + 32]) / s)) for b in range(max(1, c.N // 32)))
        point = min(float(np.min(np.max(K[:, j0:j0 + 256, None] * al[None, j0:j0 + 256] / s[:, None, :], axis=0))) for j0 in range(0, c.N, 256))
        out["shares"] = (full * nblk, point)
    return out


def figures_line(c, g):
    f = g["form"]
    drops = " ".join(f"{k} {v:.2e}" for k, v in g["drops"].items())
    faults = min(g["faults"].items(), key=lambda kv: kv[1])
    return (f"{case_id(c)}: {f.kernel} qb{f.QB} nqb{f.nqb} s{f.S} chunk{f.chunk} nb{list(f.nb)} last{f.last}: e_full {g['e_full']:.2e}, without {drops or '-'}, "
            f"smallest fault {faults[0]} {faults[1]:.2e}, claims {list(g['claims'])}, bar {g['bar']:.2e}" + (f", shares {g['shares'][0]:.2f} / nblk, {g['shares'][1]:.2e}" if "shares" in g else ""))


# ---- the checks -------------------------------------------------------------------------------------------------------
def test_form_boundaries():
    f = mean_mfma_form(200, 300, 9, 3)
    assert (f.kernel, f.QB, f.nqb, f.S, f.chunk, f.nb, f.last) == ("bf16", 2, 2, 1, 512, (7,), 8)
    f = mean_mfma_form(200, 300, 9, 4)
    assert (f.QB, f.nqb, f.S, f.nb) == (1, 3, 1, (7,))
    f = mean_mfma_form(513, 300, 9, 3)
    assert (f.S, f.chunk, f.nb, f.last) == (2, 512, (16, 1), 1)
    f = mean_mfma_form(2144, 300, 9, 3)
    assert (f.S, f.chunk, f.nb, f.last) == (5, 512, (16, 16, 16, 16, 3), 32)
    for M, P in ((BIG3, 3), (BIG4, 4), (262144, 3), (131072, 4)):
        f = mean_mfma_form(2048, M, 9, P)
        assert (f.S, f.chunk, f.nb) == (1, 2048, (64,)), (M, P)
    assert mean_mfma_form(2048, 262144 - 256, 9, 3).S == 2 and mean_mfma_form(2048, 131072 - 128, 9, 4).S == 2      # 1023 workgroups: two chunks
    assert mean_mfma_form(2049, BIG3, 9, 3).nb == (48, 17)                          # never more than 2048 points per chunk
    for D, kernel in ((9, "bf16"), (14, "bf16"), (15, "f32"), (16, "f32")):
        f = mean_mfma_form(4100, 90000, D, 3)
        assert (f.kernel, f.nqb, f.S, f.chunk, f.nb, f.last) == (kernel, 352, 3, 1536, (48, 48, 33), 4)
        assert f.rounds == ((512, 512, 512), (512, 512, 512), (512, 512, 4))
    f = mean_mfma_form(1024, 262144, 16, 3)
    assert (f.S, f.chunk, f.rounds) == (1, 1024, ((512, 512),))
    f = mean_mfma_form(1, 1, 1, 8)
    assert (f.QB, f.nqb, f.S, f.chunk, f.nb, f.last) == (1, 1, 1, 512, (1,), 1)
    assert [mean_mfma_form(n, 300, 9, 3).nb for n in (20, 32, 33, 64, 544, 608)] == [(1,), (1,), (2,), (2,), (16, 1), (16, 3)]
    assert [mean_mfma_form(200, m, 9, 3).nqb for m in (1, 255, 256, 257)] == [1, 1, 1, 2] and [mean_mfma_form(200, m, 9, 4).nqb for m in (255, 256, 257)] == [2, 2, 3]
    assert mean_mfma_form(2600, 300, 16, 5).rounds == ((512,),) * 5 + ((40,),)
    # the last workgroup partly and wholly past M in both layouts (group A): waves of 32 QB queries
    for P in (3, 4):
        f = mean_mfma_form(200, 300, 9, P)
        waves = [(f.nqb - 1) * 128 * f.QB + w * 32 * f.QB for w in range(4)]            # first query of every wave of the last workgroup
        assert any(q < 300 < q + 32 * f.QB for q in waves) and any(q >= 300 for q in waves), P
    assert form_words(200, 300, 9, 3) == ["bf16", "200", "300", "9", "3", "qb2", "nqb2", "s1", "chunk512"]


def test_every_instantiation_and_edge_is_a_case():
    forms = {c: mean_mfma_form(c.N, c.M, c.D, c.P) for c in ALL_CASES}
    assert {(f.kernel, c.P) for c, f in forms.items()} == {(k, P) for k in ("bf16", "f32") for P in range(1, 9)}
    bf = [f for f in forms.values() if f.kernel == "bf16"]
    assert {1, 2, 3, 7, 16, 33, 48, 64} <= {n for f in bf for n in f.nb}               # single, even, odd, the longest chunk
    assert {1, 4, 8, 20, 32} <= {f.last for f in bf}
    assert {c.D for c, f in forms.items() if f.kernel == "bf16"} >= {1, 6, 7, 8, 13, 14}  # `1`, |u_q|^2 at k = 6, 7 / 7, 8 / 8, 9 / 14, 15
    assert any(f.kernel == "f32" and len(r) > 1 for f in forms.values() for r in f.rounds) and any(f.kernel == "f32" and f.rounds[-1][-1] == 4 for f in forms.values())
    assert all(forms[c].S >= 5 for c in GROUPS["G"])


def test_split_and_butterfly_restatements():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4096) * 60.0).astype(f32)
    x0, x1, x2 = split3_parts(x)
    assert np.array_equal((x0.astype(f64) + x1) + x2, x.astype(f64))
    # the halving butterfly and the plain one add the same 32 values, in different trees
    v = rng.random((1, 32, 1)).astype(f32)
    a, b = v, v
    for _ in range(5):
        h = a.shape[1] // 2
        a, b = a[:, :h] + a[:, h:], b[:, 0::2] + b[:, 1::2]
    assert abs(float(a[0, 0, 0]) - float(v.astype(f64).sum())) < 1e-5 and abs(float(b[0, 0, 0]) - float(v.astype(f64).sum())) < 1e-5


@pytest.mark.parametrize("c", [c for c in ALL_CASES if c.regime in ("gate", "gate0")], ids=case_id)
def test_gate_operands(c):
    ops = case_operands(c)
    r2 = np.concatenate([norm2(scaled(ops[k], ops["ls"], ops["center"])) for k in ("X", "Xq")]).astype(f64)
    print(f"{case_id(c)}: |u|^2 in [{r2.min():.2f}, {r2.max():.2f}]")
    if c.regime == "gate":
        assert 48.0 <= r2.min() and r2.max() <= 64.0
        assert np.array_equal(ops["X"], case_operands(c._replace(regime="gate0"))["X"])
    else:
        assert r2.max() < 4.0


@pytest.mark.parametrize("c", ALL_CASES, ids=case_id)
def test_bar_lies_above_the_emulation_and_under_every_fault(c):
    g = case_figures(c)
    print(figures_line(c, g))
    print("   faults: " + ", ".join(f"{k} {v:.2e}" for k, v in g["faults"].items()))
    bar = g["bar"]
    assert 0.0 < g["e_full"] and bar <= 4.0 * g["e_full"]
    for name, shift in g["faults"].items():
        assert shift > 4.0 * bar, (name, shift, bar)
    assert set(g["inert"]) == ({"a0b1", "a1b1", "a0b2"} if c.N == 1 and g["drops"] else set())     # a single point is the centre: b = (0.., 0, 1), b1 = b2 = 0
    for d in FIRST_ORDER:
        if g["drops"] and d not in g["inert"]:
            assert g["drops"][d] > 4.0 * bar, (d, g["drops"][d], bar)
    for d in g["claims"]:
        assert g["drops"][d] >= 8.0 * g["e_full"] and bar <= g["drops"][d] / 4.0
    if c.regime == "share":
        ops = case_operands(c)
        assert float(ops["alpha"].min()) >= 0.5 and float(ops["alpha"].max()) <= 1.5
        block, point = g["shares"]
        assert block >= 0.25, block
        if c.M >= 64:
            assert point > 8.0 * bar, (point, bar)


def test_operands_are_what_the_docstring_says():
    c = Case("share", 200, 300, 9, 3)
    ops = case_operands(c)
    assert ops["X"].dtype == f32 and ops["Xq"].dtype == f32 and ops["alpha"].dtype == f32
    assert ops["X"].shape == (200, 9) and ops["Xq"].shape == (300, 9) and ops["alpha"].shape == (200, 3)
    assert len(set(ops["ym"])) == 3 and len(set(ops["ys"])) == 3 and np.allclose(ops["center"], ops["X"].astype(f64).mean(axis=0))
    mean, den = (t.numpy() for t in mean_reference(ops, ops["Xq"], False))
    from oracle import gp_oracle as O
    want = ops["ym"] + ops["ys"] * (O.rbf_cross(ops["Xq"].astype(f64), ops["X"].astype(f64), ops["ls"], SF2) @ ops["alpha"].astype(f64))
    assert np.max(np.abs(mean - want)) < 1e-12 * np.max(np.abs(want)) and np.all(den > 0)
    s = (mean - ops["ym"]) / ops["ys"]
    assert np.all(s > 0) and len(np.unique(s)) == s.size
    sg = case_operands(Case("signed", 600, 300, 9, 3))
    assert 0.3 < float((sg["alpha"] < 0).mean()) < 0.7 and float(np.abs(sg["alpha"]).min()) >= 0.5
    s0 = case_operands(Case("signed0", 600, 300, 9, 5))
    assert all((s0["X"] == q).all(axis=1).any() for q in s0["Xq"][:8])
