"""Host side of tests/test_gpu_moments_forms.py: the cases, their operands, an extended-precision reference, the mirror of the
launch rules and the bars of the moment-matching kernels (K11: gpk_moments.hip) - nothing here needs a GPU.

Entries: query = gpk_moments_host[_multi], vjp = gpk_moments_vjp_host[_multi], chain = gpk_propagate_mm_host[_multi], chain_grad =
gpk_propagate_mm_grad_host[_multi]; `multi` picks the batch form (B single-output models), else one model with P outputs.

Operands (`case_operands`), from a seed derived from the case and not from a fitted model:
* X standard normal per model; length-scales per model and feature in [0.7, 2.5] sqrt(D); alpha: random signs, magnitude in [0.5,
  1.5] / sqrt(N); Kinv a dense symmetric matrix with entries N(0, 1) / N - no inverse of anything: E[v] = kss - sum_ij Kinv_ij L_ij
  is literal; sf2, kss, noise, y_mean, y_std distinct per model or output;
* queries 0.5 N(0, 1) in normalised units; S = c V V^T in normalised units with c from 1e-4 to 10 times the squared length-scales
  across the batch; row 0 has S = 0, row 1 a rank-1 S (nx >= 2); the strict upper triangle of the host's Sq holds other finite
  values (the lower triangle is the matrix); with a scaler, one in_scale is negative;
* seeds: gmean, gcov (not symmetric), gxcov (columns >= nx not zero) standard normal.
Clip cases: floor_ is the midpoint of the largest gap of the reference's sorted E[v] over the batch (`clip_floor`); elsewhere
floor_ lies 0.5 below the smallest E[v]: the clip decides nothing there.

Reference (`reference`): the formulas at the head of gpk_moments.hip and of its "adjoint of the moments" comment, literally, per
(query, pair), in np.longdouble: the N x N matrix L is built from M = S_x T^-1 diag(1 / (P_a + P_b)) itself (w_i . w_j = zeta_i^T M
zeta_j: no factor of M), the floor_ clip with the noise added after it.  `reference(.., ab=True)` is the same code on absolute values
with every subtraction an addition: the sum of the absolute values of the summands of every output.

Mirror (`moments_form`): mm_work, mm_query_groups and the PC choice restated, with `cus` as the log line gives it.

Bars: bar = 2^-53 phi A, A the absolute-value form of the output and phi one chain length for the whole output - the sum of
  pair sums   50 + 2 P + (tiles of the busiest workgroup) + G    (the 4 x 4 FMAs, the products with alpha or zeta, the two LDS passes
              of 16, wgt, the slot's += per tile, the finishing sum over G slots)
  row sums    min(N, 256) + nrw + 6
  exponent    (nx + D + 6) emag + EXP_ULPS,  emag the largest sum of the absolute values of the terms of an exponent
  factors     F max(|cl| + 2 zmax^2 |M|, |cm| + zmax^2 |Bm|),  F = 2 (nx + 2).  The second factor is the sensitivity: what a relative
              perturbation of 2^-53 of Bm, M = G G^T, cl and cm (matrices in the spectral norm) can move an exponent by, at most,
              whatever its signs - an analytic bound on the largest change over ALL sign patterns, computed by the reference, where
              sampling a few random patterns would give a little less and cost three more long-double passes per query (zmax the
              largest 2-norm of a scaled row, |cl| and |cm| the sums of the absolute values of their logarithms).  F is the chain
              behind an entry of a factor: at most nx FMAs, a square root and a division in mm_chol, and as many again in the
              triangular inverse and the products.  No condition number enters: the sensitivity is to perturbations of the
              factors themselves, as for every other operand of a first-order bar
  small       4 nx + 12: the nx x nx products and the scalings of the finishing launches
Every piece comes from the reference and the mirror; nothing in a bar is taken from a GPU result.

Host tests: the mirror at hand-counted switch points; the adjoint reference against central differences of the forward reference
(N <= 65, the step rule of test_moments_grad_host.by_the_step_rule); the clip gap is at least 1e6 bars wide with queries on both
sides; plain fp64 NumPy of the same formulas in three orders of the training rows (as given, reversed, tile-interleaved) within
every bar - largest error / bar over all cases and outputs: 0.143 (Sigma of the three-stage batch chain, whose bar is a few
roundings of an nx x nx composition; 0.021 over the query and adjoint cases, at N = 1, P = 5); the reference's E[v] of every clip
case stays on its side of floor_ under K^-1 x KSCALE, which the GPU test runs as "another K^-1".
A lost piece: one 64 x 64 tile (with its mirror image), one workgroup slot of a diagonal pair, one block of 256 rows or one query
group removed from the fp64 sums of the last query moves some entry of every affected output by at least 100 bars - smallest ratio
1.1e4 (one tile of 1176 at N = 3009).  This test runs on the forward query cases without a clip (at N >= 1985 on P = 1, B = 1 only:
a pass costs seconds) and removes tiles from diagonal pairs only; the adjoint and the chains run the same tile walk, slots and
query groups (one launch rule, `moments_form`), and the GPU file's wrong builds 1, 2 and 4 show what a lost piece does to them.
The chain gradient's central differences cover dx0, dU and dSigma0 of the last rollout of one single-model chain and of one batch
chain with a scaler and `coord` a permutation.  The long-double sums at N = 1985 and 3009 run in one order of plain NumPy only
and take 2 .. 7 s each; everything else takes well under a second, the batch chain's differences 3 s.
The chains (group D) are checked stage by stage from their own traj[h] and Sigma[h]: see `chain_run`."""
import math
import zlib
from collections import namedtuple

import numpy as np
import pytest

from test_small_refs import EXP_ULPS, U, padded, ratio

HP = np.longdouble
MM_TILE, MM_CH, MM_MAXG, MM_ROWS = 64, 12, 512, 256
CUS = 256                 # an MI355X; the GPU tests take the count from the log line
KSCALE = 1.0 + 2.0 ** -20  # the clip cases run once more on K^-1 times this: no E[v] changes its side of floor_ (`test_clip_gap`)

Case = namedtuple("Case", "group entry multi B P D nx N R pad noisy clip sq cap scaler null H rows s0 qn")


def _c(group, entry, N, P=1, D=3, nx=2, R=3, B=1, multi=None, pad=0, noisy=0, clip=0, sq=1, cap=0, scaler=0, null="", H=0, rows="R",
       s0=1, qn=1):
    return Case(group, entry, bool(B > 1 if multi is None else multi), B, P, D, nx, N, R, pad, noisy, clip, sq, cap, scaler, null, H, rows,
                s0, qn)


def case_id(c):
    s = f"{c.group}-{c.entry}{'-multi' if c.multi else ''}-B{c.B}-P{c.P}-D{c.D}-nx{c.nx}-N{c.N}-R{c.R}"
    s += (f"-ldk+{c.pad}" if c.pad else "") + ("-noise" if c.noisy else "") + ("-clip" if c.clip else "") + ("" if c.sq else "-noS")
    s += (f"-cap{c.cap}" if c.cap else "") + ("-scaler" if c.scaler else "") + (f"-no{c.null}" if c.null else "")
    if c.H:
        s += f"-H{c.H}-rows{c.rows}" + ("" if c.s0 else "-noS0") + ("" if c.qn else "-noQ")
    return s


GROUPS = {
    # forward, one model: all 16 P without and with the query dimension; N at every tile and row-block edge; G capped (N = 1985, 3009);
    # nx != P; R and the caps giving NQ in {1, 2, 3, R}; the pitch; the noise; the clip; Sq NULL
    "A": [_c("A", "query", 65, P=p, D=3, nx=3, R=5, cap=cap, noisy=p % 2, pad=2 * (p % 3 == 0)) for p in range(1, 17) for cap in (1, 0)]
         + [_c("A", "query", n, P=p, pad=2 * (n % 2)) for n in (1, 63, 64, 65, 128, 255, 256, 257, 300) for p in (1, 5)]
         + [_c("A", "query", n, P=p, R=2) for n in (1985, 3009) for p in (1, 3)]
         + [_c("A", "query", 65, P=2, D=1, nx=1), _c("A", "query", 65, P=2, D=16, nx=1), _c("A", "query", 65, P=2, D=16, nx=16),
            _c("A", "query", 65, P=2, D=5, nx=2), _c("A", "query", 65, P=5, D=7, nx=3, noisy=1)]
         + [_c("A", "query", 65, P=2, R=1), _c("A", "query", 65, P=2, R=2), _c("A", "query", 65, P=2, R=5, cap=3),
            _c("A", "query", 65, P=2, R=5, cap=2), _c("A", "query", 65, P=2, R=32), _c("A", "query", 65, P=2, R=32, cap=3)]
         + [_c("A", "query", 130, P=3, R=5, clip=1), _c("A", "query", 65, P=1, R=5, clip=1, noisy=1), _c("A", "query", 130, P=2, sq=0)],
    # forward, batch: B = 1 .. 8 (pair_of, the row-vector slots); G U = 540; G capped; a negative in_scale; the clip on some models
    "B": [_c("B", "query", 65, B=b, multi=True, noisy=b % 2, pad=2 * (b % 3 == 0)) for b in range(1, 9)]
         + [_c("B", "query", 257, B=8, R=2), _c("B", "query", 1985, B=2, D=2, nx=1, R=1), _c("B", "query", 130, B=3, scaler=1),
            _c("B", "query", 65, B=4, R=4, clip=1, scaler=1)],
    # adjoint
    "C": [_c("C", "vjp", 65, P=p, D=3, nx=3, noisy=p % 2) for p in (1, 2, 8, 9, 16)]
         + [_c("C", "vjp", 65, P=2, D=d, nx=nx) for d, nx in ((1, 1), (5, 3), (16, 16), (16, 1))]
         + [_c("C", "vjp", 130, P=2, null=s, pad=2) for s in ("gmean", "gcov", "gxcov")]
         + [_c("C", "vjp", 130, P=3, R=5, clip=1), _c("C", "vjp", 1985, P=1, D=2, nx=1, R=1), _c("C", "vjp", 65, B=3, scaler=1, noisy=1),
            _c("C", "vjp", 65, B=2, R=4, clip=1), _c("C", "vjp", 65, P=2, R=5, cap=3), _c("C", "vjp", 65, P=2, sq=0)],
}
ALL_CASES = [c for g in GROUPS.values() for c in g]
# group E: six calls of different entries in a row on one handle
SEQUENCE = [GROUPS["A"][30], GROUPS["C"][1], GROUPS["B"][4], GROUPS["A"][33], GROUPS["C"][14], GROUPS["A"][0]]


# ---- the launch rules, restated ---------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


Form = namedtuple("Form", "G U NQ split nrw NV PC NVadj tpw groups")


def moments_form(B, P, D, nx, N, R, cus=CUS, cap=0):
    """mm_work, mm_query_groups and the PC choice of mg_launch: G workgroups per pair, U pairs, NQ query groups with their query
    ranges, nrw row blocks, NV sums of the forward and of the adjoint, tpw the tiles of the busiest workgroup of the pair launch."""
    nt = _ceil(N, MM_TILE)
    lower = nt * (nt + 1) // 2
    G = min(lower, MM_MAXG)
    Up = B * (B + 1) // 2
    wgs = G * Up
    if wgs >= MM_MAXG:
        nq = 1
    else:
        nq = 2 * cus // wgs
        if cap >= 1 and nq > cap:
            nq = cap
        nq = max(1, min(nq, R))
    groups = [(z * R // nq, (z + 1) * R // nq) for z in range(nq)]
    tiles = nt * nt if B > 1 else lower
    return Form(G, Up, nq, int(nq > 1), _ceil(N, MM_ROWS), 1 + P * (P + 1) // 2, 1 if P == 1 else 8 if P <= 8 else 16,
                1 + D + nx * (nx + 1) // 2, _ceil(tiles, G), groups)


def case_form(c, cus=CUS):
    return moments_form(c.B, c.P, c.D, c.nx, c.N, c.R, cus, c.cap)


def case_lines(c, cus=CUS):
    """The words of the library's GPKMM lines (option gram_log) of one call of a query or vjp case."""
    f = case_form(c, cus)
    head = [str(v) for v in (c.B, c.P, c.D, c.nx, c.N, c.R)] + [f"cus{cus}", f"g{f.G}", f"u{f.U}", f"nq{f.NQ}", f"split{f.split}", f"nrw{f.nrw}"]
    lines = [["fwd"] + head + [f"nv{f.NV}", f"p{c.P}"]]
    if c.entry == "vjp":
        lines.append(["adj"] + head + [f"nv{f.NVadj}", f"pc{f.PC}"])
    return lines


# ---- operands -----------------------------------------------------------------------------------------------------------------
_ops = {}


def case_operands(c):
    """The host arrays of a case (fp64, read-only, built once).  The seed ignores the options that change no value (cap, pad)."""
    key = c._replace(cap=0, pad=0, group="", entry="", null="", clip=0, H=0, rows="", s0=0, qn=0)
    if key in _ops:
        return _ops[key]
    rng = np.random.default_rng(zlib.crc32(repr(tuple(key)).encode()))
    B, P, D, nx, N, R = c.B, c.P, c.D, c.nx, c.N, c.R
    NO = B * P
    o = {"X": [rng.standard_normal((N, D)) for _ in range(B)],
         "ls": rng.uniform(0.7, 2.5, (B, D)) * math.sqrt(D),
         "alpha": [rng.choice([-1.0, 1.0], (N, P)) * rng.uniform(0.5, 1.5, (N, P)) / math.sqrt(N) for _ in range(B)],
         "sf2": 0.6 + 0.13 * np.arange(B) + rng.uniform(0, 0.1, B), "kss": 0.9 + 0.11 * np.arange(B) + rng.uniform(0, 0.1, B),
         "noise": 0.02 + 0.007 * np.arange(B), "ym": 0.3 * rng.standard_normal(NO), "ys": 0.5 + 0.2 * np.arange(NO) + rng.uniform(0, 0.1, NO)}
    o["Kinv"] = []
    for _ in range(B):
        A = np.tril(rng.standard_normal((N, N))) / N
        o["Kinv"].append(A + np.tril(A, -1).T)
    if c.scaler:
        o["shift"] = 0.2 * rng.standard_normal(D)
        o["scale"] = rng.uniform(0.7, 1.4, D)
        o["scale"][0] = -o["scale"][0]
    else:
        o["shift"], o["scale"] = np.zeros(D), np.ones(D)
    z = 0.5 * rng.standard_normal((R, D))
    o["Xq"] = o["shift"] + o["scale"] * z
    Sn = np.zeros((R, nx, nx))
    cs = np.geomspace(1e-4, 10.0, max(R - 1, 1))
    l0 = o["ls"][0][:nx]
    for r in range(1, R):
        V = rng.standard_normal((nx, nx if not (r == 1 and nx >= 2) else 1)) / math.sqrt(nx)
        Sn[r] = cs[r - 1] * (l0[:, None] * (V @ V.T) * l0[None, :])
    Sraw = Sn * np.outer(o["scale"][:nx], o["scale"][:nx])
    Sraw = np.tril(Sraw) + np.tril(Sraw, -1).transpose(0, 2, 1)          # (exactly symmetric: the lower triangle is the matrix)
    o["S"] = Sraw
    o["Sq"] = np.tril(Sraw) + np.triu(1.0 + rng.uniform(0, 1, (R, nx, nx)), 1)      # what the host entry is given
    o["gmean"], o["gcov"], o["gxcov"] = rng.standard_normal((R, NO)), rng.standard_normal((R, NO, NO)), rng.standard_normal((R, NO, D))
    for v in o.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    _ops[key] = o
    return o


def kinv_device_image(c, b):
    """The Np x ldk array the device gets: the lower triangle inside N, NaN above the diagonal, in rows and columns >= N and in the
    pitch columns."""
    N, Np = c.N, padded(c.N)
    img = np.full((Np, Np + c.pad), np.nan)
    K = case_operands(c)["Kinv"][b]
    il = np.tril_indices(N)
    img[il] = K[il]
    return img


# ---- the reference --------------------------------------------------------------------------------------------------------------
def _inv(A):
    """Gauss-Jordan inverse of a small matrix in its own dtype and its pivots (those of an SPD matrix are the squares of its
    Cholesky factor's diagonal)."""
    n = len(A)
    M = np.concatenate([A.copy(), np.eye(n, dtype=A.dtype)], axis=1)
    piv = np.zeros(n, dtype=A.dtype)
    for c in range(n):
        piv[c] = M[c, c]
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, n:], piv


def _norm2(A):
    """The spectral norm of a small matrix (fp64 is enough for a bar)."""
    return float(np.linalg.norm(np.asarray(A, dtype=np.float64), 2))


def _pairs(B):
    return [(a, b) for a in range(B) for b in range(a + 1)]


class Model:
    """The operands of a case in one dtype, the training rows in the order `perm`; `rows_i`, `rows_j`: the rows of the pair sums that
    are kept (None: all), `rows_m`: those of the row sums."""

    def __init__(self, c, dt=HP, perm=None):
        o = case_operands(c)
        self.c, self.dt = c, np.dtype(dt)
        pm = np.arange(c.N) if perm is None else perm
        cv = lambda a: np.asarray(a, dtype=dt)
        self.X = [cv(x[pm]) for x in o["X"]]
        self.al = [cv(a[pm]) for a in o["alpha"]]
        self.K = [cv(k[np.ix_(pm, pm)]) for k in o["Kinv"]]
        self.ls, self.sf2, self.kss, self.noise, self.ym, self.ys = (cv(o[k]) for k in ("ls", "sf2", "kss", "noise", "ym", "ys"))
        self.shift, self.scale = cv(o["shift"]), cv(o["scale"])
        self.z = (cv(o["Xq"]) - self.shift) / self.scale
        nx = c.nx
        self.S = (cv(o["S"]) if c.sq else np.zeros((c.R, nx, nx), dtype=dt)) / np.outer(self.scale[:nx], self.scale[:nx])


def query_sums(m, r, ab=False, rows_i=None, rows_j=None, rows_m=None):
    """The sums of query r in normalised units: Em (NO), Cs (NO, nx) = sum alpha l nu_x, Bm per model, pv per pair ((P, P): alpha_a^T L
    alpha_b), Ks per model (sum Kinv L), and what the bars need (emag, fact).  ab: absolute values throughout."""
    c, dt = m.c, m.dt
    B, P, D, nx, N = c.B, c.P, c.D, c.nx, c.N
    A = np.abs if ab else (lambda x: x)
    z, S = m.z[r], m.S[r]
    half = dt.type(0.5)
    out = dict(Em=[], Cs=[], Bm=[], pv={}, Ks=[], M={}, emag=0.0, fact=0.0)
    sel = slice(None) if rows_m is None else rows_m
    for b in range(B):
        ls2 = m.ls[b] ** 2
        nu = (m.X[b] - z)[sel]
        T = S + np.diag(ls2[:nx])
        Bm, piv = _inv(T)
        cm = np.log(m.sf2[b]) - half * (np.sum(np.log(piv)) - np.sum(np.log(ls2[:nx])))
        quad = np.einsum("nd,de,ne->n", nu[:, :nx], Bm, nu[:, :nx]) + np.sum(nu[:, nx:] ** 2 / ls2[nx:], axis=1)
        l = np.exp(cm - half * quad)
        al = A(m.al[b][sel])
        out["Em"] += list(al.T @ l)
        out["Cs"] += list((al * l[:, None]).T @ A(nu[:, :nx]))
        out["Bm"].append(Bm)
        zmax = float(np.max(np.sqrt(np.sum(nu[:, :nx] ** 2, axis=1)), initial=0.0))
        cabs = float(abs(np.log(m.sf2[b])) + half * (np.sum(np.abs(np.log(piv))) + np.sum(np.abs(np.log(ls2[:nx])))))
        out["emag"] = max(out["emag"], cabs + float(np.max(half * np.abs(quad), initial=0.0)))
        out["fact"] = max(out["fact"], cabs + zmax ** 2 * _norm2(Bm))
    out["Em"], out["Cs"] = np.array(out["Em"], dtype=dt), np.array(out["Cs"], dtype=dt).reshape(B * P, nx)
    si = slice(None) if rows_i is None else rows_i
    sj = slice(None) if rows_j is None else rows_j
    for a, b in _pairs(B):
        pa, pb = 1 / m.ls[a] ** 2, 1 / m.ls[b] ** 2
        dd = 1 / (pa[:nx] + pb[:nx])
        T = S + np.diag(dd)
        Ti, piv = _inv(T)
        Mm = S @ Ti * dd[None, :]                                   # M = S_x T^-1 diag(1 / (P_a + P_b))
        logR = np.sum(np.log(piv)) - np.sum(np.log(dd))             # log |R| = log |T| + sum log (P_a + P_b)
        nua, nub = (m.X[a] - z)[si], (m.X[b] - z)[sj]
        za, zb = nua * pa, nub * pb
        qa, wa = np.sum(nua * za, axis=1), np.einsum("nd,de,ne->n", za[:, :nx], Mm, za[:, :nx])
        qb, wb = np.sum(nub * zb, axis=1), np.einsum("nd,de,ne->n", zb[:, :nx], Mm, zb[:, :nx])
        lama = np.log(m.sf2[a]) - half * qa + half * wa
        lamb = np.log(m.sf2[b]) - half * qb + half * wb
        L = np.exp(-half * logR + lama[:, None] + lamb[None, :] + za[:, :nx] @ Mm @ zb[:, :nx].T)
        out["pv"][(a, b)] = A(m.al[a][si]).T @ (L @ A(m.al[b][sj]))
        if a == b:
            Ka = m.K[a] if rows_i is None and rows_j is None else m.K[a][np.ix_(np.arange(N)[si], np.arange(N)[sj])]
            out["Ks"].append(np.sum(A(Ka) * L))
        out["M"][(a, b)] = (Mm, dd, L, za, zb)
        clabs = float(half * (np.sum(np.abs(np.log(piv))) + np.sum(np.abs(np.log(dd)))))
        ea = abs(float(np.log(m.sf2[a]))) + float(np.max(half * qa + half * np.abs(wa), initial=0.0))
        eb = abs(float(np.log(m.sf2[b]))) + float(np.max(half * qb + half * np.abs(wb), initial=0.0))
        out["emag"] = max(out["emag"], clabs + 2.0 * float(ea + eb))
        zmax = max(float(np.max(np.sqrt(np.sum(za[:, :nx] ** 2, axis=1)), initial=0.0)), float(np.max(np.sqrt(np.sum(zb[:, :nx] ** 2, axis=1)), initial=0.0)))
        out["fact"] = max(out["fact"], clabs + 2.0 * zmax ** 2 * _norm2(Mm))
    return out


def ev_of(m, s):
    """E[v_b] per model, unclipped (normalised units)."""
    return np.array([m.kss[b] - s["Ks"][b] for b in range(m.c.B)], dtype=m.dt)


def assemble(m, r, s, floor, ab=False, clipped=None):
    """mean (NO), cov (NO, NO), xcov (NO, D) of query r in raw units from its sums; ab: from the absolute sums (clipped: the side of
    each model's E[v], from the signed reference)."""
    c, dt = m.c, m.dt
    B, P, D, nx = c.B, c.P, c.D, c.nx
    NO = B * P
    A = np.abs if ab else (lambda x: x)
    Em = s["Em"]
    V = np.zeros((NO, NO), dtype=dt)
    for a, b in _pairs(B):
        blk = s["pv"][(a, b)]
        if B > 1:
            V[a, b] = V[b, a] = blk[0, 0]
        else:
            V[:] = np.tril(blk) + np.tril(blk, -1).T
    V = V + np.outer(Em, Em) if ab else V - np.outer(Em, Em)
    for o in range(NO):
        b = o // P if B > 1 else 0
        if ab:
            var = A(dt.type(floor)) if clipped[b] else A(m.kss[b]) + s["Ks"][b]
        else:
            ev = m.kss[b] - s["Ks"][b]
            var = ev if ev > floor else dt.type(floor)
        if c.noisy:
            var = var + m.noise[b]
        V[o, o] += var
    ys = A(m.ys)
    cov = V * np.outer(ys, ys)
    mean = A(m.ym) + ys * Em
    xc = np.zeros((NO, D), dtype=dt)
    for o in range(NO):
        b = o // P if B > 1 else 0
        xc[o, :nx] = A(m.S[r]) @ (A(s["Bm"][b]) @ s["Cs"][o]) * ys[o] * A(m.scale[:nx])
    return dict(mean=mean, cov=cov, xcov=xc)


def seeds_of(c):
    o = case_operands(c)
    return {k: (None if c.null == k else o[k]) for k in ("gmean", "gcov", "gxcov")}


def adjoint(m, r, s, floor, ab=False, keep=None, sd=None):
    """dXq (D) and dSq (nx, nx) of query r: the formulas of the "adjoint of the moments" comment, literally.  keep: [E[v_b] > floor]
    per model (ab: from the signed reference); sd: the raw seeds of the row (gmean (NO), gcov (NO, NO), gxcov (NO, >= nx)) or None
    per seed, default: the case's own."""
    c, dt = m.c, m.dt
    B, P, D, nx = c.B, c.P, c.D, c.nx
    NO = B * P
    A = np.abs if ab else (lambda x: x)
    half = dt.type(0.5)
    if sd is None:
        sd = {k: (None if v is None else v[r]) for k, v in seeds_of(c).items()}
    ys, sc = A(m.ys), A(m.scale)
    z0 = lambda shape: np.zeros(shape, dtype=dt)
    eb = z0(NO) if sd["gmean"] is None else A(np.asarray(sd["gmean"], dt)) * ys
    gc = z0((NO, NO)) if sd["gcov"] is None else np.asarray(sd["gcov"], dt)
    Vb = A(half * (gc + gc.T)) * np.outer(ys, ys)
    Cb = z0((NO, nx)) if sd["gxcov"] is None else A(np.asarray(sd["gxcov"], dt)[:, :nx]) * ys[:, None] * sc[None, :nx]
    z, S = m.z[r], A(m.S[r])
    Em = s["Em"]
    eh = eb + 2 * (Vb @ Em) if ab else eb - 2 * (Vb @ Em)
    mb, Sb = z0(D), z0((nx, nx))
    I = np.eye(nx, dtype=dt)
    for b in range(B):
        ls2 = m.ls[b] ** 2
        Bm = A(s["Bm"][b])
        nu = m.X[b] - z
        quad = np.einsum("nd,de,ne->n", nu[:, :nx], s["Bm"][b], nu[:, :nx]) + np.sum(nu[:, nx:] ** 2 / ls2[nx:], axis=1)
        _, piv = _inv(m.S[r] + np.diag(ls2[:nx]))
        l = np.exp(np.log(m.sf2[b]) - half * (np.sum(np.log(piv)) - np.sum(np.log(ls2[:nx]))) - half * quad)
        nu = A(nu)
        al = A(m.al[b])
        os_ = range(b * P, b * P + P) if B > 1 else range(P)
        tb = np.array([Bm @ (S @ Cb[o]) for o in os_], dtype=dt).reshape(len(os_), nx)
        w = l * np.sum(al * (eh[list(os_)][None, :] + nu[:, :nx] @ tb.T), axis=1)
        W0, W1, W2 = np.sum(w), nu.T @ w, (nu[:, :nx].T * w) @ nu[:, :nx]
        mb[:nx] += Bm @ W1[:nx]
        mb[nx:] += W1[nx:] / ls2[nx:]
        t1, t2 = half * (Bm @ W2 @ Bm), half * W0 * Bm
        Sb += t1 + t2 if ab else t1 - t2
        for i, o in enumerate(os_):
            mb[:nx] += (tb[i] * Em[o]) if ab else -(tb[i] * Em[o])
            t_o = Bm @ ((al[:, i] * l) @ nu[:, :nx])
            Sb += np.outer(Cb[o] + tb[i] if ab else Cb[o] - tb[i], t_o)
    for a, b in _pairs(B):
        Mm, dd, L, za, zb = s["M"][(a, b)]
        Mm, za, zb = A(Mm), A(za), A(zb)
        pab = 1 / dd
        if B > 1:
            cij = (1 if a == b else 2) * Vb[a, b] * np.outer(A(m.al[a][:, 0]), A(m.al[b][:, 0]))
            kap = Vb[a, a] if a == b else 0
        else:
            cij = A(m.al[0]) @ Vb @ A(m.al[0]).T
            kap = np.trace(Vb)
        if a == b and keep[a]:
            cij = cij + kap * A(m.K[a]) if ab else cij - kap * m.K[a]
        W = cij * L
        wi, wj = W.sum(axis=1), W.sum(axis=0)
        A0 = W.sum()
        A1 = za.T @ wi + zb.T @ wj
        cross = za[:, :nx].T @ W @ zb[:, :nx]
        A2 = (za[:, :nx].T * wi) @ za[:, :nx] + (zb[:, :nx].T * wj) @ zb[:, :nx] + cross + cross.T
        RiT = I + pab[:, None] * Mm if ab else I - pab[:, None] * Mm      # R^-T = I - P_ab G G^T
        mb[:nx] += RiT @ A1[:nx]
        mb[nx:] += A1[nx:]
        last = half * A0 * (RiT * pab[None, :])                          # (S + P_ab^-1)^-1 = R^-T P_ab
        Sb += half * (RiT @ A2 @ RiT.T) + (last if ab else -last)
    return dict(dXq=mb / sc, dSq=half * (Sb + Sb.T) / np.outer(sc[:nx], sc[:nx]))


def outputs_of(c):
    return ("mean", "cov", "xcov") + (("dXq", "dSq") if c.entry == "vjp" else ())


def phi_of(c, s, form):
    """The chain length of a case's outputs at one query (the module docstring)."""
    F = 2.0 * (c.nx + 2)
    return (50 + 2 * c.P + form.tpw + form.G) + (min(c.N, MM_ROWS) + form.nrw + 6) + ((c.nx + c.D + 6) * s["emag"] + EXP_ULPS) + F * s["fact"] \
        + 4 * c.nx + 12


_refs = {}


def reference(c):
    """{output: (fp64 value, long-double value, bar)} over the R queries, "_ev": E[v] (R, B) unclipped, "_floor", "_keep" (R, B);
    computed once per case."""
    key = c._replace(cap=0, pad=0, group="")
    if key in _refs:
        return _refs[key]
    m, form = Model(c), case_form(c)
    sums = [query_sums(m, r) for r in range(c.R)]
    ev = np.array([ev_of(m, s) for s in sums])
    floor = clip_floor(ev) if c.clip else float(np.min(ev)) - 0.5
    keep = ev > floor
    res = {k: [] for k in outputs_of(c)}
    bars = {k: [] for k in outputs_of(c)}
    for r, s in enumerate(sums):
        sa = query_sums(m, r, ab=True)
        phi = U * phi_of(c, s, form)
        val, av = assemble(m, r, s, floor), assemble(m, r, sa, floor, ab=True, clipped=~keep[r])
        if c.entry == "vjp":
            val.update(adjoint(m, r, s, floor, keep=keep[r]))
            av.update(adjoint(m, r, sa, floor, ab=True, keep=keep[r]))
        for k in res:
            res[k].append(val[k])
            bars[k].append(np.asarray(phi * av[k], dtype=np.float64))
    out = {k: (np.array(res[k], dtype=np.float64), np.array(res[k], dtype=HP), np.array(bars[k])) for k in res}
    out.update(_ev=ev, _floor=float(floor), _keep=keep, _sums=sums)
    _refs[key] = out
    return out


def clip_floor(ev):
    """The midpoint of the largest gap of the sorted E[v] of a batch."""
    v = np.sort(np.asarray(ev, dtype=np.float64).ravel())
    i = int(np.argmax(np.diff(v)))
    return 0.5 * (v[i] + v[i + 1])


def ev_bar(c, r):
    """The bar of E[v_b] of query r per model: 2^-53 phi (|kss| + sum |Kinv| L)."""
    m = Model(c)
    s, sa = reference(c)["_sums"][r], query_sums(m, r, ab=True)
    return np.array([U * phi_of(c, s, case_form(c)) * float(abs(m.kss[b]) + sa["Ks"][b]) for b in range(c.B)])


# ---- plain fp64 NumPy in three orders of the training rows -------------------------------------------------------------------------
def orders(N):
    nt = _ceil(N, MM_TILE)
    tile = np.array(sorted(range(N), key=lambda i: (i % MM_TILE, i // MM_TILE)))
    return {"rows": np.arange(N), "reversed": np.arange(N)[::-1], "tiles": tile}


def fp64_outputs(c, perm):
    ref = reference(c)
    m = Model(c, np.float64, perm)
    res = {k: [] for k in outputs_of(c)}
    for r in range(c.R):
        s = query_sums(m, r)
        val = assemble(m, r, s, ref["_floor"])
        if c.entry == "vjp":
            val.update(adjoint(m, r, s, ref["_floor"], keep=ref["_keep"][r]))
        for k in res:
            res[k].append(val[k])
    return {k: np.array(v) for k, v in res.items()}


def worst(c, got):
    """{output: (e / bar, e, bar)} at the worst entry of `got` against the reference."""
    ref = reference(c)
    out = {}
    for k in outputs_of(c):
        e = np.asarray(np.abs(np.asarray(got[k], dtype=HP) - ref[k][1]), dtype=np.float64)
        q = ratio(e, ref[k][2])
        i = np.unravel_index(int(np.argmax(q)), q.shape)
        out[k] = (float(q[i]), float(e[i]), float(ref[k][2][i]))
    return out


HOST_CASES = [c for c in ALL_CASES]


@pytest.mark.parametrize("c", HOST_CASES, ids=case_id)
def test_fp64_numpy_is_within_every_bar(c):
    big = 0.0
    for name, perm in orders(c.N).items():
        if c.N >= 1985 and name != "reversed":      # (one order at the sizes where a pass costs seconds)
            continue
        w = worst(c, fp64_outputs(c, perm))
        big = max(big, max(v[0] for v in w.values()))
    print(f"{case_id(c)}: fp64 NumPy / bar {big:.2e}")
    assert big < 0.25, big


@pytest.mark.parametrize("c", [c for c in ALL_CASES if c.clip], ids=case_id)
def test_clip_gap(c):
    ref = reference(c)
    ev, floor = np.asarray(ref["_ev"], dtype=np.float64), ref["_floor"]
    bars = np.array([ev_bar(c, r) for r in range(c.R)])
    gap = np.min(np.abs(ev - floor) / bars)
    print(f"{case_id(c)}: floor {floor:.4f}, {int((ev > floor).sum())} above, {int((ev < floor).sum())} below, nearest E[v] {gap:.2e} bars away")
    assert (ev > floor).any() and (ev < floor).any() and gap >= 0.5e6      # (the gap is twice the distance to its midpoint)
    # K^-1 times KSCALE: E[v] = kss - KSCALE sum Kinv L stays on its side, still 1e5 bars from floor_, and moves by more than 100 bars
    m = Model(c)
    ev2 = np.array([[float(m.kss[b] - HP(KSCALE) * s["Ks"][b]) for b in range(c.B)] for s in ref["_sums"]])
    gap2, moved = np.min(np.abs(ev2 - floor) / bars), np.min(np.abs(ev2 - ev) / bars)
    print(f"{case_id(c)}: under K^-1 x (1 + 2^-20) the nearest E[v] is {gap2:.2e} bars away, every E[v] moves by at least {moved:.2e} bars")
    assert np.array_equal(ev2 > floor, ev > floor) and gap2 >= 1e5 and moved >= 100.0


@pytest.mark.parametrize("c", [c for c in ALL_CASES if not c.clip], ids=case_id)
def test_clip_decides_nothing_elsewhere(c):
    ref = reference(c)
    assert ref["_keep"].all() and np.min(np.asarray(ref["_ev"], dtype=np.float64)) - ref["_floor"] >= 0.49


def test_mirror_at_hand_counted_switch_points():
    f = moments_form
    # nt = 31 | 32: 496 | 528 lower tiles, G capped at 512, sixteen workgroups walk a second tile
    assert f(1, 1, 3, 2, 1984, 2).G == 496 and f(1, 1, 3, 2, 1984, 2).tpw == 1 and f(1, 1, 3, 2, 1984, 2).NQ == 1      # 2 * 256 // 496 = 1
    assert f(1, 1, 3, 2, 1985, 2).G == 512 and f(1, 1, 3, 2, 1985, 2).tpw == 2 and f(1, 1, 3, 2, 1985, 2).split == 0
    assert f(1, 1, 3, 2, 3009, 2).tpw == 3      # nt = 48: 1176 lower tiles over 512 workgroups
    # G U = 511 | 512 cannot be reached with G = nt (nt + 1) / 2: B = 8 at N = 257 has 15 x 36 = 540, at N = 256 10 x 36 = 360
    assert f(8, 1, 3, 2, 257, 2, cap=0).NQ == 1 and f(8, 1, 3, 2, 257, 2).tpw == 2       # 25 tiles over 15 workgroups
    assert f(8, 1, 3, 2, 256, 2).NQ == 1                                                  # 512 // 360 = 1
    assert f(7, 1, 3, 2, 256, 2).NQ == 1 and f(6, 1, 3, 2, 256, 2).NQ == 2               # 10 x 28 = 280 -> 1; 10 x 21 = 210 -> 2
    # 2 cus / wgs = 1 | 2 through cus
    assert f(1, 1, 3, 2, 65, 5, cus=2).NQ == 1 and f(1, 1, 3, 2, 65, 5, cus=3).NQ == 2 and f(1, 1, 3, 2, 65, 5, cus=1).NQ == 1
    # ... and the rule `G U >= 512 -> 1` apart from a count that 2 cus / (G U) limits: with 496 CUs, 992 // 496 = 2 at N = 1984, and
    # N = 1985 (G = 512) has one group although 992 // 512 = 1 too; with 512 CUs 1024 // 512 = 2 would split it - it must not
    assert f(1, 1, 3, 2, 1984, 2, cus=496).NQ == 2 and f(1, 1, 3, 2, 1985, 2, cus=496).NQ == 1
    assert f(1, 1, 3, 2, 1985, 2, cus=512).NQ == 1 and f(1, 1, 3, 2, 1985, 4, cus=2048).NQ == 1 and f(1, 1, 3, 2, 1984, 4, cus=2048).NQ == 4
    # capped by R and by the option; R / NQ not integral
    assert f(1, 1, 3, 2, 65, 5).NQ == 5 and f(1, 1, 3, 2, 65, 5, cap=3).groups == [(0, 1), (1, 3), (3, 5)]
    assert f(1, 1, 3, 2, 65, 32).NQ == 32 and f(1, 1, 3, 2, 65, 32, cap=1).split == 0 and f(1, 1, 3, 2, 65, 1).NQ == 1
    # P = 1 | 2, 8 | 9
    assert [f(1, p, 3, 2, 65, 1).PC for p in (1, 2, 8, 9, 16)] == [1, 8, 8, 16, 16]
    assert f(1, 5, 3, 2, 65, 1).NV == 16 and f(1, 16, 16, 16, 65, 1).NV == 137 and f(1, 16, 16, 16, 65, 1).NVadj == 153
    assert f(1, 2, 5, 3, 65, 1).NVadj == 12 and f(1, 1, 3, 2, 257, 1).nrw == 2 and f(1, 1, 3, 2, 256, 1).nrw == 1


def test_every_switch_point_is_a_case():
    forms = [(c, case_form(c)) for c in ALL_CASES]
    assert {c.P for c in GROUPS["A"]} == set(range(1, 17)) and {c.B for c in GROUPS["B"]} == set(range(1, 9))
    assert {f.tpw for _, f in forms} >= {1, 2, 3} and {f.NQ for c, f in forms if c.group == "A"} >= {1, 2, 3, 5, 32}
    assert any(f.G * f.U >= 512 and f.U > 1 for _, f in forms) and {f.PC for c, f in forms if c.entry == "vjp"} == {1, 8, 16}
    assert any(f.NVadj % MM_CH == 0 for c, f in forms if c.entry == "vjp") and any(f.NVadj == 153 for _, f in forms)


# ---- the adjoint reference against central differences of the forward reference -----------------------------------------------------
@pytest.mark.parametrize("c", [GROUPS["C"][1], GROUPS["C"][6], GROUPS["C"][14]], ids=case_id)
def test_adjoint_reference_matches_central_differences(c):
    from test_moments_grad_host import by_the_step_rule
    assert c.N <= 65 and not c.clip
    o, ref = case_operands(c), reference(c)
    r = c.R - 1
    sd = seeds_of(c)
    nx, D = c.nx, c.D

    def loss(dq, dS):
        m = Model(c)
        m.z = m.z.copy()
        m.S = m.S.copy()
        m.z[r] = m.z[r] + np.asarray(dq, HP) / m.scale
        m.S[r] = m.S[r] + np.asarray(dS, HP) / np.outer(m.scale[:nx], m.scale[:nx])
        v = assemble(m, r, query_sums(m, r), ref["_floor"])
        gc = np.asarray(sd["gcov"][r], HP)
        return np.sum(sd["gmean"][r] * v["mean"]) + np.sum((gc + gc.T) / 2 * v["cov"]) + np.sum(sd["gxcov"][r][:, :nx] * v["xcov"][:, :nx])

    l0 = float(loss(np.zeros(D), np.zeros((nx, nx))))
    eps = np.finfo(HP).eps
    fd_q = lambda h: np.array([float((loss(h * e, np.zeros((nx, nx))) - loss(-h * e, np.zeros((nx, nx)))) / (2 * h)) for e in np.eye(D)])
    by_the_step_rule(f"{case_id(c)}: dXq", ref["dXq"][0][r], fd_q, eps, l0)

    def fd_S(h):
        out = np.zeros((nx, nx))
        for i in range(nx):
            for j in range(i + 1):
                E = np.zeros((nx, nx))
                E[i, j] = E[j, i] = 1.0
                d = float((loss(np.zeros(D), h * E) - loss(np.zeros(D), -h * E)) / (2 * h))
                out[i, j] = out[j, i] = d if i == j else d / 2
        return out
    by_the_step_rule(f"{case_id(c)}: dSq", ref["dSq"][0][r], fd_S, eps, l0)


# ---- a lost piece moves every affected output by at least 100 bars -------------------------------------------------------------------
def _lost(c, what):
    """The largest |change| / bar per output when one piece of the sums of the last query is missing."""
    ref, form = reference(c), case_form(c)
    r = c.R - 1
    m = Model(c, np.float64)
    full = full0 = query_sums(m, r)
    N = c.N
    nt = _ceil(N, MM_TILE)
    if what == "rows":                   # one block of 256 rows of the row pass
        keep = np.arange(min(N, MM_ROWS), N) if N > MM_ROWS else np.arange(0)
        part = query_sums(m, r, rows_m=keep)
        full = dict(full, Em=part["Em"], Cs=part["Cs"])
    else:                                # the last tile (ti, tj) of workgroup slot g (tile) or all of its tiles (slot), diagonal pairs
        tiles = [(ti, tj) for ti in range(nt) for tj in range(ti + 1)]
        g = (len(tiles) - 1) % form.G
        mine = tiles[g::form.G] if what == "slot" else [tiles[-1]]
        pv = {k: v.copy() for k, v in full["pv"].items()}
        Ks = list(full["Ks"])
        for ti, tj in mine:
            I, J = np.arange(ti * 64, min(N, ti * 64 + 64)), np.arange(tj * 64, min(N, tj * 64 + 64))
            for (I_, J_) in ([(I, J)] if ti == tj else [(I, J), (J, I)]):
                sub = query_sums(m, r, rows_i=I_, rows_j=J_)
                for a in range(c.B):
                    pv[(a, a)] = pv[(a, a)] - sub["pv"][(a, a)]
                    Ks[a] = Ks[a] - sub["Ks"][a]
        full = dict(full, pv=pv, Ks=Ks)
    want = assemble(m, r, full0, ref["_floor"])
    got = assemble(m, r, full, ref["_floor"])
    return {k: float(np.max(ratio(np.abs(got[k] - want[k]), ref[k][2][r]))) for k in ("mean", "cov", "xcov")}


LOST_CASES = [c for c in ALL_CASES if c.entry == "query" and not c.clip and (c.N < 1985 or (c.P == 1 and c.B == 1))]


@pytest.mark.parametrize("c", LOST_CASES, ids=case_id)
def test_a_lost_piece_moves_every_affected_output(c):
    small = np.inf
    for what, outs in (("tile", ("cov",)), ("slot", ("cov",)), ("rows", ("mean", "cov", "xcov"))):
        moved = _lost(c, what)
        for k in outs:
            if k == "xcov" and (not c.sq or c.R == 1):
                continue                 # (S = 0, as in row 0 of every batch: xcov is exactly zero)
            small = min(small, moved[k])
    # one query group: the outputs of its queries are missing altogether
    ref = reference(c)
    for k in ("mean", "cov"):
        small = min(small, float(np.max(ratio(np.abs(ref[k][0][c.R - 1]), ref[k][2][c.R - 1]))))
    print(f"{case_id(c)}: a lost piece moves an entry by at least {small:.2e} bars")
    assert small >= 100.0, small


# ---- group D: the two chain entries and their two gradient entries -------------------------------------------------------------------
# Stage h of a chain is the query entry at ([traj[h], U[h]], Sigma[h]) followed by the composition x+ = x + lin q + E mean, Sigma+ = A0
# Sigma A0^T + A0 Cx E^T + E Cx^T A0^T + E V E^T + Q.  `chain_run` checks a chain stage by stage FROM THE CHAIN'S OWN traj[h] and
# Sigma[h] (fp64 numbers, exact inputs of the stage), so no error is carried from stage to stage and every bar is that of one stage:
# the stage outputs' bars as above; traj and Sigma: 2^-53 (2 nx + D + 8) (absolute-value form of the composition) + the stage outputs'
# bars carried through it.  The backward sweep is linear in (lam, Lam): its absolute-value form carried through all H stages is the
# sum over every path of summands, and a path meets each stage's roundings once, so bar = 2^-53 (sum_h phi_h + H (4 nx + 2 D + 12)) A.
GROUPS["D"] = [
    _c("D", e, 65, P=2, D=3, nx=2, H=1, rows="1", s0=0, qn=0) for e in ("chain", "chain_grad")] + [
    _c("D", e, 65, P=2, D=3, nx=2, H=3, rows="R", noisy=1) for e in ("chain", "chain_grad")] + [
    _c("D", e, 65, P=3, D=3, nx=3, H=3, rows="mix", qn=0, pad=2) for e in ("chain", "chain_grad")] + [
    _c("D", e, 1985, P=1, D=2, nx=1, R=1, H=1, rows="R") for e in ("chain", "chain_grad")] + [
    _c("D", e, 65, B=2, D=5, nx=4, H=3, rows="R", scaler=1) for e in ("chain", "chain_grad")] + [
    _c("D", e, 65, B=3, D=5, nx=5, H=1, rows="1", s0=0, noisy=1) for e in ("chain", "chain_grad")]
ALL_CASES += GROUPS["D"]
_chain_ops = {}


def chain_operands(c):
    """x0 (rows, nx), U (rows, H, nu), lin (nx, D), Sigma0 (rows, nx, nx) and Q (nx, nx) - their lower triangles are the matrices,
    the strict upper triangles hold other values -, coord (a permutation of B of the nx coordinates on the multi entries), and the
    seeds gx (H + 1, R, nx), gS (H + 1, R, nx, nx), not symmetric."""
    key = c._replace(cap=0, pad=0, group="", entry="")
    if key in _chain_ops:
        return _chain_ops[key]
    rng = np.random.default_rng(zlib.crc32(("chain" + repr(tuple(key))).encode()))
    nx, D, R, H = c.nx, c.D, c.R, c.H
    rows = {"R": (R, R, R), "1": (1, 1, 1), "mix": (1, R, 1)}[c.rows]
    o = {"x0": 0.3 * rng.standard_normal((rows[0], nx)), "U": 0.3 * rng.standard_normal((rows[1], H, D - nx)),
         "lin": 0.05 * rng.standard_normal((nx, D)), "gx": rng.standard_normal((H + 1, R, nx)), "gS": rng.standard_normal((H + 1, R, nx, nx))}
    spd = lambda: (lambda V: 0.05 * (V @ V.T) / nx)(rng.standard_normal((nx, nx)))
    junk = lambda: np.triu(1.0 + rng.uniform(0, 1, (nx, nx)), 1)
    o["Sigma0"] = np.array([np.tril(spd()) + junk() for _ in range(rows[2])]) if c.s0 else None
    o["Q"] = np.tril(0.2 * spd()) + junk() if c.qn else None
    o["coord"] = [int(v) for v in rng.permutation(nx)[:c.B]] if c.multi else list(range(c.P))
    o["rows"] = rows
    _chain_ops[key] = o
    return o


def _sym_lower(A):
    return np.tril(A) + np.tril(A, -1).swapaxes(-1, -2)


def chain_lines(c, cus=CUS):
    f = moments_form(c.B, c.P, c.D, c.nx, c.N, c.R, cus, c.cap)
    head = [str(v) for v in (c.B, c.P, c.D, c.nx, c.N, c.R)] + [f"cus{cus}", f"g{f.G}", f"u{f.U}", f"nq{f.NQ}", f"split{f.split}", f"nrw{f.nrw}"]
    lines = [["fwd"] + head + [f"nv{f.NV}", f"p{c.P}"]] * c.H
    return lines + ([["adj"] + head + [f"nv{f.NVadj}", f"pc{f.PC}"]] * c.H if c.entry == "chain_grad" else [])


def chain_outputs(c):
    return ("traj", "Sigma", "mean", "cov", "xcov") + (("dU", "dx0", "dSigma0") if c.entry == "chain_grad" else ())


def chain_run(c, dt, floor, given=None, bars=True):
    """The chain of a case in dtype dt.  given None: the recursion itself (what plain NumPy computes).  given {traj, Sigma}: every
    stage from given's own traj[h], Sigma[h] - returns ({output: value}, {output: bar})."""
    o, co = case_operands(c), chain_operands(c)
    dt = np.dtype(dt)
    nx, D, R, H, NO = c.nx, c.D, c.R, c.H, c.B * c.P
    cv = lambda a: np.asarray(a, dtype=dt)
    lin, coord, form = cv(co["lin"]), co["coord"], case_form(c)
    A0 = np.eye(nx, dtype=dt) + lin[:, :nx]
    Qm = cv(_sym_lower(co["Q"])) if c.qn else np.zeros((nx, nx), dtype=dt)
    Ue = np.broadcast_to(cv(co["U"]), (R, H, D - nx))
    traj, Sig = np.zeros((H + 1, R, nx), dtype=dt), np.zeros((H + 1, R, nx, nx), dtype=dt)
    traj[0] = np.broadcast_to(cv(co["x0"]), (R, nx))
    if c.s0:
        Sig[0] = np.broadcast_to(cv(_sym_lower(co["Sigma0"])), (R, nx, nx))
    val = {"traj": traj, "Sigma": Sig, "mean": np.zeros((H, R, NO), dtype=dt), "cov": np.zeros((H, R, NO, NO), dtype=dt),
           "xcov": np.zeros((H, R, NO, D), dtype=dt)}
    bar = {k: np.zeros(v.shape) for k, v in val.items()}
    E = np.zeros((nx, NO), dtype=dt)
    for oo, cc in enumerate(coord):
        E[cc, oo] = 1
    m = Model(c, dt)
    stages = []
    for h in range(H):
        xin = cv(given["traj"][h]) if given else traj[h]
        Sin = cv(given["Sigma"][h]) if given else Sig[h]
        q = np.concatenate([xin, Ue[:, h]], axis=1)
        m.z = (q - m.shift) / m.scale
        m.S = Sin / np.outer(m.scale[:nx], m.scale[:nx])
        stages.append((m.z.copy(), m.S.copy(), q))
        for r in range(R):
            s = query_sums(m, r)
            v = assemble(m, r, s, floor)
            assert all(ev_of(m, s) > floor)
            for k in ("mean", "cov", "xcov"):
                val[k][h, r] = v[k]
            Cx = v["xcov"][:, :nx]
            F = A0 @ Cx.T @ E.T
            traj[h + 1, r] = xin[r] + lin @ q[r] + E @ v["mean"]
            Sig[h + 1, r] = _sym_lower(A0 @ Sin[r] @ A0.T + F + F.T + E @ v["cov"] @ E.T + Qm)
            if dt == HP and bars:
                av = assemble(m, r, query_sums(m, r, ab=True), floor, ab=True, clipped=np.zeros(c.B, dtype=bool))
                phi = U * phi_of(c, s, form)
                for k in ("mean", "cov", "xcov"):
                    bar[k][h, r] = np.asarray(phi * av[k], dtype=np.float64)
                aA, aE = np.abs(A0), np.abs(E)
                ax = np.abs(xin[r]) + np.abs(lin) @ np.abs(q[r]) + aE @ av["mean"]
                bar["traj"][h + 1, r] = np.asarray(U * (D + 4) * ax + aE @ bar["mean"][h, r], dtype=np.float64)
                aF = aA @ av["xcov"][:, :nx].T @ aE.T
                aS = aA @ np.abs(Sin[r]) @ aA.T + aF + aF.T + aE @ av["cov"] @ aE.T + np.abs(Qm)
                bF = aA @ bar["xcov"][h, r][:, :nx].T @ aE.T
                bar["Sigma"][h + 1, r] = np.asarray(U * (2 * nx + D + 8) * aS + bF + bF.T + aE @ bar["cov"][h, r] @ aE.T, dtype=np.float64)
    if given:
        traj[0], Sig[0] = cv(given["traj"][0]), cv(given["Sigma"][0])      # (slot 0 is the input itself)
    if c.entry != "chain_grad":
        return val, bar
    gx, gS = cv(co["gx"]), cv(co["gS"])
    half = dt.type(0.5)
    val.update(dU=np.zeros((R, H, D - nx), dtype=dt), dx0=np.zeros((R, nx), dtype=dt), dSigma0=np.zeros((R, nx, nx), dtype=dt))
    bar.update({k: np.zeros(val[k].shape) for k in ("dU", "dx0", "dSigma0")})
    for r in range(R):
        for ab in ((False, True) if dt == HP else (False,)):
            A = np.abs if ab else (lambda x: x)
            lam, Lam = A(gx[H, r]), A(half * (gS[H, r] + gS[H, r].T))
            aA0, alin = A(A0), A(lin)
            phis, dUs = 0.0, np.zeros((H, D - nx), dtype=dt)
            for h in range(H - 1, -1, -1):
                m.z, m.S = stages[h][0], stages[h][1]
                s = query_sums(m, r)
                sd = dict(gmean=lam[coord], gcov=Lam[np.ix_(coord, coord)], gxcov=2 * (Lam[coord] @ aA0))
                g = adjoint(m, r, query_sums(m, r, ab=True) if ab else s, floor, ab=ab, keep=np.ones(c.B, dtype=bool), sd=sd)
                gq = alin.T @ lam + g["dXq"]
                gq[:nx] += lam
                dUs[h] = gq[nx:]
                lam = A(gx[h, r]) + gq[:nx]
                Lam = A(half * (gS[h, r] + gS[h, r].T)) + aA0.T @ Lam @ aA0 + g["dSq"]
                phis += phi_of(c, s, form) + 4 * nx + 2 * D + 12
            if ab:
                bar["dU"][r], bar["dx0"][r], bar["dSigma0"][r] = (np.asarray(U * phis * a, dtype=np.float64) for a in (dUs, lam, Lam))
            else:
                val["dU"][r], val["dx0"][r], val["dSigma0"][r] = dUs, lam, Lam
    return val, bar


_chain_host = {}


def chain_host(c):
    """(the chain in plain fp64 NumPy, floor_): floor_ lies 0.5 below the smallest E[v] along it - the clip decides nothing."""
    key = c._replace(cap=0, pad=0, group="")
    if key not in _chain_host:
        o, co = case_operands(c), chain_operands(c)
        val, _ = chain_run(c._replace(entry="chain"), np.float64, -1e300)
        m = Model(c, np.float64)
        evs = []
        for h in range(c.H):
            q = np.concatenate([val["traj"][h], np.broadcast_to(co["U"], (c.R, c.H, c.D - c.nx))[:, h]], axis=1)
            m.z, m.S = (q - m.shift) / m.scale, val["Sigma"][h] / np.outer(m.scale[:c.nx], m.scale[:c.nx])
            evs += [ev_of(m, query_sums(m, r)) for r in range(c.R)]
        floor = float(np.min(evs)) - 0.5
        _chain_host[key] = (chain_run(c, np.float64, floor)[0], floor)
    return _chain_host[key]


def check_chain(c, got):
    """{output: (e / bar, e, bar)} at the worst entry of a chain's outputs, every stage checked from got's own traj and Sigma."""
    ref, bars = chain_run(c, HP, chain_host(c)[1], given=got)
    out = {}
    for k in chain_outputs(c):
        e = np.asarray(np.abs(np.asarray(got[k], dtype=HP) - ref[k]), dtype=np.float64)
        if e.size == 0:                 # (dU without controls)
            continue
        q = ratio(e, bars[k])
        i = np.unravel_index(int(np.argmax(q)), q.shape)
        out[k] = (float(q[i]), float(e[i]), float(bars[k][i]))
    return out


@pytest.mark.parametrize("c", GROUPS["D"], ids=case_id)
def test_fp64_numpy_chain_is_within_every_bar(c):
    w = check_chain(c, chain_host(c)[0])
    print(f"{case_id(c)}: fp64 NumPy / bar " + ", ".join(f"{k} {v[0]:.2e}" for k, v in w.items()))
    assert max(v[0] for v in w.values()) < 0.25, w


@pytest.mark.parametrize("c", [GROUPS["D"][3], GROUPS["D"][9]], ids=case_id)
def test_chain_gradient_reference_matches_central_differences(c):
    """dx0, dU and dSigma0 of the long-double sweep against central differences of the long-double chain's cost sum gx . traj + gS .
    Sigma: one model with two outputs, and a batch of two models behind a scaler with `coord` a permutation into nx = 4."""
    from test_moments_grad_host import by_the_step_rule
    assert c.entry == "chain_grad" and c.s0 and c.rows == "R"
    co, floor = chain_operands(c), chain_host(c)[1]
    val, _ = chain_run(c, HP, floor)
    gx, gS = co["gx"], co["gS"]
    key = c._replace(cap=0, pad=0, group="", entry="")

    def cost(dx, dU, dS=0):
        keep = _chain_ops[key]
        _chain_ops[key] = dict(keep, x0=np.asarray(keep["x0"], HP) + dx, U=np.asarray(keep["U"], HP) + dU,
                               Sigma0=_sym_lower(np.asarray(keep["Sigma0"], HP)) + dS)
        try:
            v, _ = chain_run(c._replace(entry="chain"), HP, floor, bars=False)
        finally:
            _chain_ops[key] = keep
        return np.sum(gx * v["traj"]) + np.sum((gS + gS.swapaxes(-1, -2)) / 2 * v["Sigma"])

    z_x, z_u = np.zeros(co["x0"].shape, dtype=HP), np.zeros(co["U"].shape, dtype=HP)
    l0 = float(cost(z_x, z_u))

    def unit(shape, i):
        e = np.zeros(shape, dtype=HP)
        e.flat[i] = 1
        return e
    # (the last rollout: every rollout runs the same code)
    ix = range(z_x.size - c.nx, z_x.size)
    iu = range(z_u.size - z_u.shape[1] * z_u.shape[2], z_u.size)
    fd_x = lambda h: np.array([float((cost(h * unit(z_x.shape, i), z_u) - cost(-h * unit(z_x.shape, i), z_u)) / (2 * h)) for i in ix])
    fd_u = lambda h: np.array([float((cost(z_x, h * unit(z_u.shape, i)) - cost(z_x, -h * unit(z_u.shape, i))) / (2 * h)) for i in iu])
    by_the_step_rule(f"{case_id(c)}: dx0", np.asarray(val["dx0"], float).ravel()[list(ix)], fd_x, np.finfo(HP).eps, l0)
    by_the_step_rule(f"{case_id(c)}: dU", np.asarray(val["dU"], float).ravel()[list(iu)], fd_u, np.finfo(HP).eps, l0)
    nx = c.nx

    def fd_S(h):         # (the pair (i, j), (j, i) moves together: dS_ij + dS_ji)
        out = np.zeros((c.R, nx, nx))
        for r in (c.R - 1,):
            for i in range(nx):
                for j in range(i + 1):
                    E = np.zeros((c.R, nx, nx), dtype=HP)
                    E[r, i, j] = E[r, j, i] = 1
                    d = float((cost(z_x, z_u, h * E) - cost(z_x, z_u, -h * E)) / (2 * h))
                    out[r, i, j] = out[r, j, i] = d if i == j else d / 2
        return out
    got = np.zeros((c.R, nx, nx))
    got[c.R - 1] = np.asarray(val["dSigma0"], float)[c.R - 1]
    by_the_step_rule(f"{case_id(c)}: dSigma0", got, fd_S, np.finfo(HP).eps, l0)
