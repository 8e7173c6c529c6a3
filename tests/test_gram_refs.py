"""The references and launch-rule restatements of tests/test_gpu_gram_forms.py, checked here without a GPU:

* `rbf_panel`: the RBF block in torch fp64 on any device - exact differences of the length-scale-divided coordinates, squares
  summed feature by feature, `exp` last - against `oracle.gp_oracle` and against an mpmath evaluation of a sample.  Measured
  here (sf2 = 1.3, inputs and length-scales as the GPU module draws them, 160 entries per D): 1.5e-16, 1.2e-16,
  1.7e-16, 1.4e-16 and 2.9e-16 * sf2 from the 40-digit value for D = 1, 9, 16, 17 and 64, so the GPU module's fp64 bar of
  1e-13 * sf2 is more than 300 times the reference's own error;
* `gram_form`, `mean_form`: the launch rules of gpk_gram and gpk_predict_mean / gpk_predict_mean_multi (gpk_gram.hip), asserted
  at the sizes where the form changes;
* `exp_table`: exp(-i^2 / 8192) from mpmath at 40 digits as a double and the rest the double leaves, with the range each entry
  falls in;
* `decode_split2_panel`: the chunk layout stated above cross_split2_kernel, against a panel encoded from the same formula.

NumPy, torch (CPU) and mpmath only."""
import numpy as np
import pytest

from oracle import gp_oracle as O

TS = 64                 # tile edge of the Gram kernels
STRIP_MAX_D = 16        # one feature chunk: the strip kernel; more: one tile per workgroup
STREAM_NP = 16384       # streaming stores from this padded size


def padded(n):
    return (int(n) + 127) // 128 * 128


# ---- the references ---------------------------------------------------------------------------------------------------
def rbf_panel(Xa, Xb, ls, sf2):
    """sf2 exp(-|xa / ls - xb / ls|^2 / 2) as an (na, nb) torch float64 tensor on the device of `Xa`: the coordinates are divided by
    the length-scale first, differenced exactly, the squares added feature by feature, `exp` applied last (in place: one
    (na, nb) array and one difference array alive at a time)."""
    import torch
    Xa = torch.as_tensor(Xa, dtype=torch.float64)
    Xb = torch.as_tensor(Xb, dtype=torch.float64, device=Xa.device)
    l = torch.as_tensor(np.asarray(ls, dtype=np.float64), device=Xa.device)
    A, B = Xa / l, Xb / l
    d2 = torch.zeros((A.shape[0], B.shape[0]), dtype=torch.float64, device=Xa.device)
    for d in range(A.shape[1]):
        df = A[:, d, None] - B[None, :, d]
        d2.addcmul_(df, df)
        del df
    return d2.mul_(-0.5).exp_().mul_(float(sf2))


def case_inputs(N, D, seed=0):
    """(X, ls) as every group of the GPU module draws them unless it says otherwise: standard normal rows and
    ls = 0.7 sqrt(D) (1 + 0.02 d), which keeps the squared distance O(1) at every D."""
    rng = np.random.default_rng(1000 * D + seed)
    return rng.standard_normal((N, D)), 0.7 * np.sqrt(D) * (1.0 + 0.02 * np.arange(D))


def exp_table(nmax):
    """exp(-i^2 / 8192), i = 0 .. nmax, from mpmath at 40 digits: (hi, lo, cls) - hi the value rounded to double, lo the rest
    (value - hi, as a double: hi + lo is the value to 2^-105), cls 0 where the value is a normal double (>= 2^-1022), 1 where it
    lies below that and the argument is still inside the routine's clamp (x >= -800: gradual underflow, down to 0), 2 where the
    argument is under the clamp (x < -800: exactly 0 is expected).  Below 2^-1022 `hi` is rounded once, to a whole number of
    least subnormals, and `lo` is the rest in units of the least subnormal (within +-0.5)."""
    import mpmath as mp
    hi, lo, cls = np.zeros(nmax + 1), np.zeros(nmax + 1), np.zeros(nmax + 1, dtype=np.int64)
    with mp.workprec(140):
        tiny, unit = mp.ldexp(1, -1022), mp.ldexp(1, -1074)
        for i in range(nmax + 1):
            x = -mp.mpf(i * i) / 8192
            v = mp.exp(x)
            if v >= tiny:
                hi[i] = float(v)
                lo[i] = float(v - mp.mpf(hi[i]))
            else:
                u = mp.nint(v / unit)
                hi[i] = np.ldexp(float(int(u)), -1074)
                lo[i] = float(v / unit - u)                       # (in units of 2^-1074 here: a double cannot hold less)
                cls[i] = 1 if x >= -800 else 2
    return hi, lo, cls


def decode_split2_panel(raw, Mp, Np):
    """(h0, h1) as float64 [q][j] from the bytes of a fragment-order fp16 x 2 panel of Mp queries x Np training points: chunk
    (q, k16 block kb, half h, part s) at (((q / 32) KB + kb) 2 + s) 64 + h 32 + q % 32 with KB = Np / 16, eight fp16 per chunk,
    j = 16 kb + 8 h + e."""
    KB = Np // 16
    c = np.ascontiguousarray(raw).view(np.float16).reshape(-1, 8)[: Mp * KB * 4]
    q = np.arange(Mp)[:, None, None]
    kb = np.arange(KB)[None, :, None]
    h = np.arange(2)[None, None, :]
    parts = []
    for s in (0, 1):
        idx = (((q // 32) * KB + kb) * 2 + s) * 64 + h * 32 + q % 32           # [q][kb][h]
        parts.append(c[idx].astype(np.float64).reshape(Mp, Np))                # [q][kb][h][e] -> j = 16 kb + 8 h + e
    return parts[0], parts[1]


# ---- the launch rules -------------------------------------------------------------------------------------------------
def strip_count(nt, gs):
    """Workgroups of the strip kernel: tile row r has r / gs + 1 strips."""
    return sum(r // gs + 1 for r in range(nt))


def gram_form(N, D):
    """(kernel, GS, nt, grid, streaming) of gpk_gram: the strip kernel for D <= 16 - strips of 8 column tiles once that still makes
    1024 workgroups, of 2 once that makes 512, else one tile per workgroup - and the tile-per-workgroup kernel (GS reported as 0)
    beyond; streaming stores from Np = 16 384."""
    Np = padded(N)
    nt = Np // TS
    if D > STRIP_MAX_D:
        return "sym", 0, nt, nt * (nt + 1) // 2, Np >= STREAM_NP
    gs = 8 if strip_count(nt, 8) >= 1024 else 2 if strip_count(nt, 2) >= 512 else 1
    return "strip", gs, nt, strip_count(nt, gs), Np >= STREAM_NP


def mean_form(dtype, N, M, multi=False):
    """(gran, S, chunk) of gpk_predict_mean: the training set in S chunks of `chunk` rows (a multiple of `gran`) so that the grid has
    about 2048 workgroups; 32-row granules for at most 512 queries against at most 16 384 rows, 128 otherwise; fp32: chunks of at
    most 2048 rows.  multi: gpk_predict_mean_multi (always 128-row granules, no fp32 cap)."""
    nqb = (M + 511) // 512
    gran = 32 if (not multi and M <= 512 and N <= 16384) else 128
    S = (2048 + nqb - 1) // nqb
    if dtype == "f32" and not multi:
        S = max(S, (N + 2047) // 2048)
    S = max(1, min(S, (N + gran - 1) // gran, 65535))
    chunk = ((N + S - 1) // S + gran - 1) // gran * gran
    return gran, (N + chunk - 1) // chunk, chunk


def colsumsq_form(Np, Mp):
    """(S, rows_per) of gpk_colsumsq: row slabs so that the grid has about 2048 workgroups, none shorter than 64 rows."""
    nmb = Mp // 128
    S = max(1, min((2048 + nmb - 1) // nmb, Np // 64, 32768))
    rows_per = (Np + S - 1) // S
    return (Np + rows_per - 1) // rows_per, rows_per


# ---- the checks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 9, 16, 17, 64])
def test_rbf_panel_against_the_oracle_and_mpmath(D):
    import mpmath as mp
    Xa, ls = case_inputs(700, D)
    Xb = case_inputs(300, D, seed=1)[0]
    got = rbf_panel(Xa, Xb, ls, 1.3).numpy()
    assert got.shape == (700, 300)
    e = np.max(np.abs(got - O.rbf_cross(Xa, Xb, ls, 1.3)))
    K = rbf_panel(Xa, Xa, ls, 1.3).numpy()
    off = ~np.eye(700, dtype=bool)
    eg = np.max(np.abs(K - O.rbf_gram(Xa, ls, 1.3, 0.0))[off])
    assert np.array_equal(K, K.T) and np.all(np.diag(K) == 1.3)
    print(f"D {D}: rbf_panel against O.rbf_cross {e:.2e}, against O.rbf_gram {eg:.2e}")
    assert e <= 4 * np.finfo(np.float64).eps * 1.3 and eg <= 4 * np.finfo(np.float64).eps * 1.3       # the same operations: exp's last bits
    # its own error: the real-number value of the same expression on the same doubles, 40 digits
    rng = np.random.default_rng(D)
    worst = 0.0
    with mp.workdps(40):
        for a, b in zip(rng.integers(0, 700, 160), rng.integers(0, 300, 160)):
            d2 = mp.mpf(0)
            for d in range(D):
                df = mp.mpf(float(Xa[a, d])) / mp.mpf(float(ls[d])) - mp.mpf(float(Xb[b, d])) / mp.mpf(float(ls[d]))
                d2 += df * df
            want = mp.mpf(1.3) * mp.exp(-d2 / 2)
            worst = max(worst, float(abs(mp.mpf(float(got[a, b])) - want)) / 1.3)
    print(f"D {D}: rbf_panel against mpmath (160 entries): {worst:.2e} of sf2")
    assert worst < 1e-15          # two orders below the GPU module's fp64 bar of 1e-13


def test_gram_form_boundaries():
    assert gram_form(2816, 9) == ("strip", 1, 44, 990, False)
    assert gram_form(2817, 9)[:3] == ("strip", 2, 46)
    assert gram_form(7808, 16)[:3] == ("strip", 2, 122)
    assert gram_form(7809, 1)[:3] == ("strip", 8, 124)
    assert [gram_form(n, 16)[2] for n in (8064, 8192, 8320)] == [126, 128, 130] and all(gram_form(n, 3)[1] == 8 for n in (8064, 8192, 8320))
    assert [gram_form(n, 16)[2] % 8 for n in (7809, 8064, 8320)] == [4, 6, 2]          # the partial last strip group
    assert gram_form(16256, 16)[4] is False and gram_form(16257, 16)[4] is True and gram_form(16257, 16)[1] == 8
    assert gram_form(16257, 17) == ("sym", 0, 256, 256 * 257 // 2, True)
    assert gram_form(200, 17) == ("sym", 0, 4, 10, False) and gram_form(200, 16) == ("strip", 1, 4, 10, False)
    for n in (1, 64, 65, 128, 129, 1000):
        assert gram_form(n, 3)[1] == 1
    assert gram_form(3000, 9)[1] == 2
    # the grid of a strip launch: every tile of the lower triangle in exactly one strip
    for nt, gs in ((46, 2), (124, 8), (126, 8), (130, 8)):
        tiles = sum(min(gs, r - g * gs + 1) for r in range(nt) for g in range(r // gs + 1))
        assert tiles == nt * (nt + 1) // 2


def test_mean_form_boundaries():
    assert mean_form("f64", 333, 3) == (32, 11, 32) and mean_form("f64", 333, 600) == (128, 3, 128)
    assert mean_form("f64", 1000, 512)[0] == 32 and mean_form("f64", 1000, 513)[0] == 128
    assert mean_form("f64", 16384, 3)[0] == 32 and mean_form("f64", 16385, 3)[0] == 128
    # fp32: no chunk longer than 2048 rows, whatever the number of queries
    assert mean_form("f32", 5000, 3) == (32, 157, 32) and mean_form("f32", 5000, 600) == (128, 40, 128)
    assert mean_form("f64", 100000, 2000000) == (128, 1, 100096) and mean_form("f32", 100000, 2000000) == (128, 49, 2048)
    assert mean_form("f32", 5000, 2000000) == (128, 3, 1792) and mean_form("f32", 4096, 2000000) == (128, 2, 2048)
    assert mean_form("f32", 4097, 2000000)[1] == 3
    assert mean_form("f32", 333, 3, multi=True) == (128, 3, 128) and mean_form("f64", 100000, 2000000, multi=True) == (128, 1, 100096)


def test_colsumsq_form():
    assert colsumsq_form(128, 128) == (2, 64) and colsumsq_form(130, 128) == (2, 65)
    assert colsumsq_form(897, 256) == (14, 65) and colsumsq_form(1000, 384) == (15, 67) and colsumsq_form(4099, 128) == (64, 65)


def test_exp_table():
    import mpmath as mp
    hi, lo, cls = exp_table(2599)
    assert hi[0] == 1.0 and lo[0] == 0.0 and cls[0] == 0
    normal = cls == 0
    assert np.all(hi[normal] >= 2.0 ** -1022) and np.all(np.abs(lo[normal]) <= 2.0 ** -53 * hi[normal])
    assert np.max(np.abs(hi[normal] - np.exp(-np.arange(2600)[normal] ** 2 / 8192.0)) / hi[normal]) < 2.0 ** -51   # libm's exp
    # the ranges: x = -i^2 / 8192 reaches 2^-1022 at i = 2409, the clamp at i = 2560
    first_sub, first_clamp = int(np.argmax(cls == 1)), int(np.argmax(cls == 2))
    assert (first_sub, first_clamp) == (2409, 2561) and np.all(cls[first_sub:first_clamp] == 1) and np.all(cls[first_clamp:] == 2)
    assert 2560 ** 2 / 8192.0 == 800.0 and np.all(hi[cls == 2] == 0.0)
    units = np.ldexp(hi[cls == 1], 1074)
    assert np.all(units == np.rint(units)) and units[0] > 2.0 ** 51 and np.all(np.diff(units) <= 0)
    with mp.workprec(140):
        i = 2430
        assert abs(mp.exp(-mp.mpf(i * i) / 8192) / mp.ldexp(1, -1074) - mp.mpf(float(units[i - first_sub]))) <= 0.5


def test_decode_split2_panel():
    rng = np.random.default_rng(3)
    Mp, Np = 128, 384
    KB = Np // 16
    h0 = rng.standard_normal((Mp, Np)).astype(np.float16)
    h1 = (rng.standard_normal((Mp, Np)) * 2.0 ** -11).astype(np.float16)
    raw = np.full(Mp * Np * 2 + 16, np.float16(7.0), dtype=np.float16)          # (a tail the decoder must not read)
    for q in range(Mp):
        for kb in range(KB):
            for h in range(2):
                for s, part in ((0, h0), (1, h1)):
                    chunk = (((q // 32) * KB + kb) * 2 + s) * 64 + h * 32 + q % 32
                    raw[8 * chunk:8 * chunk + 8] = part[q, 16 * kb + 8 * h:16 * kb + 8 * h + 8]
    d0, d1 = decode_split2_panel(raw.view(np.uint8), Mp, Np)
    assert d0.dtype == np.float64 and d0.shape == (Mp, Np)
    assert np.array_equal(d0, h0.astype(np.float64)) and np.array_equal(d1, h1.astype(np.float64))
