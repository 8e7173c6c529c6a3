"""The references, launch-rule restatements and bars of tests/test_gpu_k5_forms.py (the 16-bit variance launches of
gpk_k5split.hip), checked here without a GPU:

* `k5_direct_form`, `k5_split_form`: the launch rules of split2_launch (fp16 x 2) and gpk_predict_var_inv_split (bf16 x 3), asserted
  at the sizes where the form changes;
* `direct_walk`, `split_walk`: the kernels' own mapping from blockIdx.x to (tile row, tile column) or idle - xcd, group, serpentine
  super-tile, band, per_pad slots, the ragged last band, the heavy-first reversal - and, for bf16 x 3, the k-range each tile runs
  over (the group's longest when the group spans at most two bands, else its own).  For every case of the GPU module: every tile
  exactly once, no live slot beyond nst, every bf16 x 3 k-range within the row's own plus at most 2048 columns (where W is zero);
* `case_operands`: X, Xq fp32 standard normal, ls = 2.5 sqrt(D) (1 + 0.02 d), sf2 = 1.3, and a DENSE lower-triangular fp32 W, exactly
  zero above the diagonal, every row (padding rows included) scaled to unit sum of squares over its live range k <= r, k < N.
  Every row then carries the same share of S_m = sum_r (sum_k W_rk K*_mk)^2 and every k16 step of a row the same share of the row:
  the smallest unit of work a kernel can lose - one k16 step of one 32-row block - is at least 512 / Np^2 of S;
* `s_reference`: S in fp64 from the fp32 operands (K* from `rbf_panel`, zero for j >= N; W as stored).  Sums of squares are compared,
  e = max_m |S_gpu - S| / S, never kss - S;
* `emulate_direct`, `emulate_split`: NumPy emulations of the two forms - fp16 x 2: per-block power-of-two scale, h0 = fp16(x s),
  h1 = fp16(x s - h0), fp32 matmuls a1 b0 + a0 b1 + a0 b0; bf16 x 3: the exact three-way split and the six products - complete, and
  with the first-order cross product a1 b0 left out;
* the bar of a case, from the reference side only: bar = min(128 / Np^2, e_cross / 4) - a quarter of the smallest fault share, and
  a quarter of the error e_cross of the emulation without a1 b0.  Asserted here for every GPU case: the complete emulation errs by
  at most bar / 8, and dropping one (32-row block, k16 step) from the reference at (0, 0), (last, 0), (last, last live) and one
  interior place moves S by more than 4 bar.  At the cases of more than 2048 queries the emulations run on the first 128 queries.
  The second-order bf16 products (a1 b1, a0 b2, a2 b0: 2^-18 each) are below the fp32 accumulation noise and cannot be told apart
  by accuracy: no bar here claims to.
  One case needs a word: N = 1 (case h).  Every live entry of W is then +-1, a1 is identically zero, and the emulation without
  a1 b0 is the complete one bit for bit: there is no such fault to stay under, and e_cross / 4 would sit under the complete
  emulation itself.  `case_bar` leaves out the other first-order product, a0 b1, where leaving out a1 b0 changes no bit.
* `decode_split2_rows`: the fragment order stated in gpk_k5split.hip for the W operand, against a panel encoded from the formula;
  `split2_scales`, `split2_parts`: the block scales (absmax_to_scale_kernel) and the two parts, restated.

Measured here (complete emulation / a1 b0 left out / the smallest of the four planted faults / bar), fp16 x 2: a 9.3e-8 / 7.0e-6 /
4.2e-4 / 1.7e-6, b 6.5e-8 / 4.9e-6 / 4.5e-4 / 1.2e-6, c 5.3e-8 / 3.9e-6 / 6.0e-4 / 9.7e-7, d 1.1e-7 / 1.4e-5 / 1.1e-3 / 3.6e-6,
e 7.9e-8 / 1.2e-5 / 8.1e-4 / 2.9e-6, f 1.0e-7 / 7.4e-6 / 2.4e-4 / 1.9e-6, g 6.6e-8 / 1.6e-5 / 9.7e-5 / 4.0e-6, h 6.9e-8 / (a0 b1)
1.4e-4 / 0.25 / 3.4e-5, i 8.9e-8 / 1.4e-5 / 2.8e-3 / 3.4e-6, the block-scale case 2.6e-7 / 3.4e-5 / 4.3e-3 / 8.5e-6; without a0 b1:
5.7e-5 .. 1.6e-4.  bf16 x 3: Np 2304 2.0e-8 / 6.0e-5 .. 6.9e-5 / 1.1e-4 / 1.5e-5 .. 1.7e-5, Np 2432 1.8e-8 / 2.5e-5 .. 3.0e-5 /
7.6e-5 / 6.3e-6 .. 7.5e-6.  The bar sits at least 18 times above the complete emulation and at least 7 times under every planted
fault; 128 / Np^2 (2.2e-5 .. 7.8e-3) is never the smaller term (every case prints its own figures).

NumPy and torch (CPU) only."""
import functools

import numpy as np
import pytest

from test_gram_refs import decode_split2_panel, padded, rbf_panel

SF2 = 1.3
EMU_MAX_M = 2048        # cases of more queries: emulations and planted faults on the first EMU_COLS queries
EMU_COLS = 128


# ---- the launch rules -------------------------------------------------------------------------------------------------
def k5_direct_form(Np, Mp, opt=0):
    """(ab, bh, per, per_pad, ntmT, nst, grid) of split2_launch: tiles of 128 ab rows - the tallest of 512 / 256 / 128 that still
    comes in at least 512 tiles, option k5_split2_tile 1: 128, 2: 512 where Np % 512 == 0, 3: 256 where Np % 256 == 0 -, bands of
    bh tile rows (1024 rows), per = bh ntn tiles per band, rounded up to whole groups of 32 (per_pad) when that idles at most an
    eighth of the slots, nst super-tiles of 32 slots, grid = nst rounded up to whole rounds of the 8 XCDs, times 32."""
    ntn = Mp // 128
    ab = 1
    if Np % 512 == 0 and (opt == 2 or (Np // 512) * ntn >= 512):
        ab = 4
    elif Np % 256 == 0 and (Np // 256) * ntn >= 512:
        ab = 2
    if opt == 1:
        ab = 1
    if opt == 3 and Np % 256 == 0:
        ab = 2
    ntmT, bh = Np // (128 * ab), 1024 // (128 * ab)
    per = bh * ntn
    pad = (per + 31) // 32 * 32
    per_pad = pad if (pad - per) * 8 <= per else per
    nfull = ntmT // bh
    hlast = ntmT - nfull * bh
    nst = (nfull * per_pad + hlast * ntn + 31) // 32
    return ab, bh, per, per_pad, ntmT, nst, (nst + 7) // 8 * 8 * 32


def k5_split_form(Np, Mp):
    """(wr, gsz, bh, ntmT, nst, grid) of gpk_predict_var_inv_split: tiles of 64 wr rows (256 when Np % 256 == 0, else 128), groups of
    32 / 64 tiles, bands of 1024 rows, no padding slots."""
    ntn = Mp // 128
    wr = 4 if Np % 256 == 0 else 2
    gsz = 64 if wr == 2 else 32
    ntmT = Np // (64 * wr)
    nst = (ntmT * ntn + gsz - 1) // gsz
    return wr, gsz, 1024 // (64 * wr), ntmT, nst, (nst + 7) // 8 * 8 * gsz


# ---- the walks --------------------------------------------------------------------------------------------------------
def _slot(blk, gsz):
    xcd, j = blk & 7, blk >> 3
    grp, slot = divmod(j, gsz)
    return grp * 8 + (7 - xcd if grp & 1 else xcd), slot


def direct_walk(Np, Mp, opt=0):
    """k5_direct_kernel's mapping: a list over blockIdx.x of None (idle) or (tm, tn, st) - tile row (heavy first: the walk's row r is
    tile row ntmT - 1 - r), tile column, super-tile."""
    ab, bh, per, per_pad, ntmT, nst, grid = k5_direct_form(Np, Mp, opt)
    ntn = Mp // 128
    nfull = ntmT // bh
    hlast = ntmT - nfull * bh
    out = []
    for blk in range(grid):
        st, slot = _slot(blk, 32)
        if st >= nst:
            out.append(None)
            continue
        t = st * 32 + slot
        band = min(t // per_pad, nfull)
        idx = t - band * per_pad
        hh = bh if band < nfull else hlast
        if idx >= hh * ntn:
            out.append(None)                   # a padding slot, or beyond the last tile
            continue
        tn = idx // hh
        out.append((ntmT - 1 - (band * bh + idx - tn * hh), tn, st))
    return out


def direct_wave_ktiles(Np, Mp, opt=0):
    """k-tiles of 16 of every wave of every tile row of the fp16 x 2 launch: {(tm, wave): nkt}."""
    ab, _, _, _, ntmT, _, _ = k5_direct_form(Np, Mp, opt)
    return {(tm, w): (tm * 128 * ab + 32 * ab * (w + 1)) // 16 for tm in range(ntmT) for w in range(4)}


def split_walk(Np, Mp):
    """k5_split_kernel's mapping: a list over blockIdx.x of None or (tm, tn, st, k columns the tile runs over, lockstep?)."""
    wr, gsz, bh, ntmT, nst, grid = k5_split_form(Np, Mp)
    ntn, tmr = Mp // 128, 64 * wr
    per, nfull, total = bh * ntn, ntmT // bh, ntmT * ntn
    hlast = ntmT - nfull * bh
    out = []
    for blk in range(grid):
        st, slot = _slot(blk, gsz)
        t = st * gsz + slot
        if st >= nst or t >= total:
            out.append(None)
            continue
        band = min(t // per, nfull)
        idx = t - band * per
        hh = bh if band < nfull else hlast
        tn = idx // hh
        tm = ntmT - 1 - (band * bh + idx - tn * hh)
        band0 = min(st * gsz // per, nfull)
        band1 = min(min(st * gsz + gsz - 1, total - 1) // per, nfull)
        lock = band1 - band0 <= 1
        rhi = ntmT - 1 - band0 * bh if lock else tm
        out.append((tm, tn, st, (rhi + 1) * tmr, lock))
    return out


# ---- the operands -----------------------------------------------------------------------------------------------------
def ls_of(D):
    return 2.5 * np.sqrt(D) * (1.0 + 0.02 * np.arange(D))


@functools.lru_cache(maxsize=None)
def _factor(N, seed):
    Np = padded(N)
    W = np.tril(np.random.default_rng(50000 + 7 * N + seed).standard_normal((Np, Np)))
    live = W[:, :N]                                                 # (k <= r by the triangle, k < N by the slice)
    W /= np.sqrt(np.einsum("ij,ij->i", live, live))[:, None]
    W = W.astype(np.float32)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def case_operands(N, M, D, seed=0):
    """(X (N, D) fp32, Xq (M, D) fp32, ls, W (Np, Np) fp32).  W depends on (N, seed) only, X on (N, D, seed)."""
    X = np.random.default_rng(51000 + 7 * N + 16 * D + seed).standard_normal((N, D)).astype(np.float32)
    Xq = np.random.default_rng(52000 + 7 * M + 16 * D + seed).standard_normal((M, D)).astype(np.float32)
    return X, Xq, ls_of(D), _factor(N, seed)


def kstar(X, Xq, ls, Np, sf2=SF2, device=None):
    """K* (M, Np) as a torch fp64 tensor: `rbf_panel` of the fp32 operands, zero for j >= N."""
    import torch
    Xq = torch.as_tensor(np.asarray(Xq, dtype=np.float64), device=device)
    K = torch.zeros((Xq.shape[0], Np), dtype=torch.float64, device=device)
    K[:, :X.shape[0]] = rbf_panel(Xq, np.asarray(X, dtype=np.float64), ls, sf2)
    return K


def s_reference(W, K):
    """S_m = sum_r (sum_k W_rk K_mk)^2 in fp64, queries in panels of 4096: W (Np, Np) any float array or tensor, K from `kstar`."""
    import torch
    Wt = torch.as_tensor(np.asarray(W, dtype=np.float64), device=K.device) if not torch.is_tensor(W) else W.to(K.device, torch.float64)
    S = torch.empty((K.shape[0],), dtype=torch.float64, device=K.device)
    for m0 in range(0, K.shape[0], 4096):
        V = K[m0:m0 + 4096] @ Wt.T
        S[m0:m0 + 4096] = (V * V).sum(dim=1)
    return S.cpu().numpy()


# ---- the split operands, restated ----------------------------------------------------------------------------------------
def split2_scales(W32):
    """One power of two per 128-row block (tril_block_absmax_kernel + absmax_to_scale_kernel): the largest s with s max <= 2^15, the
    maximum over the block's part of the lower triangle; exponent kept in [-126, 100]; 1 for a block of zeros."""
    n = W32.shape[0]
    m = np.abs(np.tril(W32)).reshape(n // 128, -1).max(axis=1).astype(np.float32)
    out = np.ones(n // 128, dtype=np.float32)
    for b, v in enumerate(m):
        u = int(v.view(np.uint32))
        if u != 0 and u < 0x7f800000:
            e = (u >> 23) - 127
            se = (15 if (u & 0x7fffff) == 0 else 14) - e
            out[b] = np.ldexp(np.float32(1.0), min(max(se, -126), 100))
    return out


def split2_parts(x32):
    """(h0, h1) fp16 of an fp32 array (already scaled): h0 = fp16(x), h1 = fp16(x - h0), both rounded to nearest."""
    h0 = x32.astype(np.float16)
    return h0, (x32 - h0.astype(np.float32)).astype(np.float16)


def k_scale_of(sf2):
    return 2.0 ** (14 - int(np.floor(np.log2(sf2))))


def _bf16_rn(x32):
    u = x32.view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) & np.uint32(0xffff0000)).view(np.float32)


def split3_parts(x32):
    """x = x0 + x1 + x2 exactly, three bf16 (held as fp32) rounded to nearest even, as split3 of gpk_k5split.hip."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    x0 = _bf16_rn(x32)
    r1 = x32 - x0
    x1 = _bf16_rn(r1)
    return x0, x1, r1 - x1


def decode_split2_rows(raw, Np):
    """(h0, h1) as float64 [row][k] from the bytes of gpk_split2_rows' destination: chunk (row, k16 block kb, half h, part s) at
    (((row / 32) KB + kb) 2 + s) 64 + h 32 + row % 32 with KB = Np / 16 - the panel layout with Np rows."""
    return decode_split2_panel(raw, Np, Np)


# ---- the emulations ---------------------------------------------------------------------------------------------------
def emulate_direct(W32, K, sf2=SF2, drop=None):
    """S of the fp16 x 2 form in NumPy: W s (one scale per 128-row block) and fp32(K*) k_scale in two fp16 parts each, V =
    a1 b0 + a0 b1 + a0 b0 by fp32 matmuls (smallest terms first), un-scaled by the two exact reciprocals, squares summed in fp64.
    drop: "a1b0" or "a0b1" leaves that product out."""
    sc = split2_scales(W32)
    a0, a1 = split2_parts(W32 * np.repeat(sc, 128)[:, None])
    b0, b1 = split2_parts(np.asarray(K, dtype=np.float64).astype(np.float32) * np.float32(k_scale_of(sf2)))
    a0, a1, b0, b1 = (p.astype(np.float32) for p in (a0, a1, b0, b1))
    V = np.zeros((W32.shape[0], b0.shape[0]), dtype=np.float32)
    if drop != "a1b0":
        V += a1 @ b0.T
    if drop != "a0b1":
        V += a0 @ b1.T
    V += a0 @ b0.T
    V *= ((np.float32(1.0) / np.repeat(sc, 128)) * (np.float32(1.0) / np.float32(k_scale_of(sf2))))[:, None]
    V = V.astype(np.float64)
    return np.einsum("rm,rm->m", V, V)


def emulate_split(W32, K, drop=None):
    """S of the bf16 x 3 form in NumPy: exact three-way splits of W and fp32(K*), the six products a2 b0, a0 b2, a1 b1, a1 b0, a0 b1,
    a0 b0 by fp32 matmuls in the kernel's order.  drop: "a1b0" leaves that product out."""
    a = split3_parts(W32)
    b = split3_parts(np.asarray(K, dtype=np.float64).astype(np.float32))
    V = np.zeros((W32.shape[0], b[0].shape[0]), dtype=np.float32)
    for i, j in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
        if drop == "a1b0" and (i, j) == (1, 0):
            continue
        V += a[i] @ b[j].T
    V = V.astype(np.float64)
    return np.einsum("rm,rm->m", V, V)


def rel_err(S_got, S):
    return float(np.max(np.abs(np.asarray(S_got, dtype=np.float64) - S) / S))


# ---- the cases of the GPU module ----------------------------------------------------------------------------------------
# fp16 x 2 (group A): name -> (N, M, D, option k5_split2_tile)
DIRECT_CASES = {
    "a": (1100, 1900, 6, 0), "b": (2100, 300, 6, 0), "c": (1200, 13100, 6, 0), "d": (700, 300, 6, 3), "e": (1500, 21800, 6, 0),
    "f": (1000, 10000, 6, 2), "g": (2000, 100, 6, 2), "h": (1, 1, 1, 0), "i": (129, 129, 16, 0),
}
# what each claims: ab, ntmT, per, per_pad (k5_direct_form), full bands, tile rows of the ragged band
DIRECT_CLAIMS = {
    "a": dict(ab=1, ntmT=9, per=120, per_pad=128, nfull=1, hlast=1), "b": dict(ab=1, ntmT=17, per=24, per_pad=24, nfull=2, hlast=1),
    "c": dict(ab=2, ntmT=5, per=412, per_pad=416, nfull=1, hlast=1), "d": dict(ab=2, ntmT=3, per=12, per_pad=12, nfull=0, hlast=3),
    "e": dict(ab=4, ntmT=3, per=342, per_pad=352, nfull=1, hlast=1), "f": dict(ab=4, ntmT=2, per=158, per_pad=160, nfull=1, hlast=0),
    "g": dict(ab=4, ntmT=4, per=2, per_pad=2, nfull=2, hlast=0), "h": dict(ab=1, ntmT=1, per=8, per_pad=8, nfull=0, hlast=1),
    "i": dict(ab=1, ntmT=2, per=16, per_pad=16, nfull=0, hlast=2),
}
# bf16 x 3 (group C): (N, M) -> (wr, the super-tiles that run in lockstep, those whose tiles keep their own k-range)
SPLIT_CASES = {
    (2250, 100): (4, [], [0]), (2250, 700): (4, [0, 1], []), (2250, 1000): (4, [0, 1, 2], []),
    (2400, 100): (2, [], [0]), (2400, 350): (2, [], [0]), (2400, 500): (2, [0, 1], []), (2400, 1000): (2, [0, 1, 2], []),
}
SPLIT_D = 6
# the block-scale case of group B: N = Np = 768, one factor per 128-row block (0: a block of zeros)
SCALE_CASE = (768, 200, 6)
SCALE_BLOCKS = (1.0, 0.0, 2.0 ** -110, 2.0 ** -90, 2.0 ** 40, 2.0 ** -160)
SCALE_WANT = (None, 1.0, 2.0 ** 100, 2.0 ** 100, None, 1.0)


def scale_case_factor():
    """(W as fp64, its fp32 rounding) of the block-scale case: the unit-row factor, block b of 128 rows times SCALE_BLOCKS[b] (exact
    in fp64).  Entries are 2^-1 .. 2^-12 or so: times 2^-110 / 2^-90 they are still normal fp32 numbers whose scale would exceed
    2^100 and is clamped there; times 2^-160 they round to zero in fp32 and meet the rule of the block of zeros (scale 1)."""
    N = SCALE_CASE[0]
    W64 = _factor(N, 0).astype(np.float64) * np.repeat(np.array(SCALE_BLOCKS), 128)[:, None]
    return W64, W64.astype(np.float32)


def _emu_cols(M):
    return M if M <= EMU_MAX_M else EMU_COLS


@functools.lru_cache(maxsize=None)
def case_bar(kind, N, M, D, seed=0, scale_case=False):
    """(bar, e_full, e_cross, which product e_cross leaves out) of a case, from the reference side only: kind "direct" or "split".
    bar = min(128 / Np^2, e_cross / 4); the emulations run on the first `_emu_cols(M)` queries."""
    X, Xq, ls, W = case_operands(N, M, D, seed)
    if scale_case:
        W = scale_case_factor()[1]
    Np = W.shape[0]
    K = kstar(X, Xq[:_emu_cols(M)], ls, Np).numpy()
    S = s_reference(W, kstar(X, Xq[:_emu_cols(M)], ls, Np))
    emu = emulate_direct if kind == "direct" else emulate_split
    full = emu(W, K)
    cross, which = emu(W, K, drop="a1b0"), "a1b0"
    if np.array_equal(cross, full):                 # a1 is identically zero on the live entries: no such fault exists (N = 1)
        assert kind == "direct"
        cross, which = emu(W, K, drop="a0b1"), "a0b1"
    e_full, e_cross = rel_err(full, S), rel_err(cross, S)
    return min(128.0 / Np ** 2, e_cross / 4.0), e_full, e_cross, which


def fault_places(N, Np):
    """(rb, kb) of the planted faults: 32-row block rb, k16 step kb - (0, 0), (last, 0), (last, last live) and an interior place."""
    last = Np // 32 - 1
    mid = last // 2
    return [(0, 0), (last, 0), (last, (N - 1) // 16), (mid, (min(32 * mid + 31, N - 1) // 16) // 2)]


def fault_shift(W, K, S, rb, kb):
    """max_m |S' - S| / S where S' is the reference without the products of rows 32 rb .. + 31 and columns 16 kb .. + 15."""
    rows, cols = slice(32 * rb, 32 * rb + 32), slice(16 * kb, 16 * kb + 16)
    W64 = np.asarray(W[rows], dtype=np.float64)
    v = W64 @ K.T                                     # (32, M)
    d = W64[:, cols] @ K[:, cols].T
    return rel_err(S - (v * v).sum(axis=0) + ((v - d) ** 2).sum(axis=0), S)


# ---- the checks -------------------------------------------------------------------------------------------------------
def test_direct_form_boundaries():
    # (ab, bh, per, per_pad, ntmT, nst, grid)
    assert k5_direct_form(1024, 10112) == (1, 8, 632, 640, 8, 20, 768)              # the headline shape under the rule: 2 x 79 < 512
    assert k5_direct_form(1024, 10112, 2) == (4, 2, 158, 160, 2, 5, 256)            # ... and as it is served (forced 512-row tiles)
    assert k5_direct_form(1536, 21888)[0] == 4 and k5_direct_form(1536, 21760)[0] == 2       # 3 x 171 = 513 / 6 x 170
    assert k5_direct_form(1536, 10880)[0] == 1 and k5_direct_form(1536, 11008)[0] == 2       # 6 x 85 = 510 / 6 x 86 = 516
    assert k5_direct_form(1280, 13184)[0] == 2 and k5_direct_form(1280, 13056)[0] == 1       # 5 x 103 = 515 / 5 x 102 = 510
    assert k5_direct_form(1280, 13184, 1)[0] == 1 and k5_direct_form(1280, 13184, 2)[0] == 2 and k5_direct_form(1280, 128, 3)[0] == 2
    assert k5_direct_form(1152, 128, 3)[0] == 1 and k5_direct_form(1152, 128, 2)[0] == 1     # neither can be forced: Np % 256 != 0
    assert k5_direct_form(2048, 128, 3)[0] == 2 and k5_direct_form(2048, 128, 2)[0] == 4 and k5_direct_form(2048, 128, 0)[0] == 1
    # per_pad: rounded up when that idles at most an eighth of the slots
    assert k5_direct_form(1024, 128 * 14)[2:4] == (112, 112) and k5_direct_form(1024, 128 * 15)[2:4] == (120, 128)   # 16 > 112 / 8, 8 <= 120 / 8
    assert k5_direct_form(1024, 128 * 28)[2:4] == (224, 224) and k5_direct_form(1024, 128 * 3)[2:4] == (24, 24)
    for name, (N, M, D, opt) in DIRECT_CASES.items():
        ab, bh, per, per_pad, ntmT, nst, grid = k5_direct_form(padded(N), padded(M), opt)
        c = DIRECT_CLAIMS[name]
        assert (ab, ntmT, per, per_pad, ntmT // bh, ntmT % bh) == (c["ab"], c["ntmT"], c["per"], c["per_pad"], c["nfull"], c["hlast"]), name
    # k5_direct_kernel<2>: by the rule (c) and by option 3 (d); <4> by the rule (e) and forced (f, g)
    assert k5_direct_form(padded(1200), padded(13100), 0)[0] == 2 and k5_direct_form(padded(700), padded(300), 0)[0] == 1
    assert k5_direct_form(padded(1000), padded(10000), 0)[0] == 1 and k5_direct_form(padded(2000), padded(100), 0)[0] == 1


def test_split_form_boundaries():
    # (wr, gsz, bh, ntmT, nst, grid)
    assert k5_split_form(2304, 128) == (4, 32, 4, 9, 1, 256) and k5_split_form(2432, 128) == (2, 64, 8, 19, 1, 512)
    assert k5_split_form(2304, 768) == (4, 32, 4, 9, 2, 256) and k5_split_form(2304, 1024) == (4, 32, 4, 9, 3, 256)
    assert k5_split_form(2432, 384)[4] == 1 and k5_split_form(2432, 512)[4] == 2 and k5_split_form(2432, 1024)[4] == 3
    assert k5_split_form(128, 128) == (2, 64, 8, 1, 1, 512) and k5_split_form(256, 128) == (4, 32, 4, 1, 1, 256)
    for (N, M), (wr, _, _) in SPLIT_CASES.items():
        assert k5_split_form(padded(N), padded(M))[0] == wr


@pytest.mark.parametrize("name", list(DIRECT_CASES))
def test_direct_walk_visits_every_tile_once(name):
    N, M, D, opt = DIRECT_CASES[name]
    Np, Mp = padded(N), padded(M)
    ab, bh, per, per_pad, ntmT, nst, grid = k5_direct_form(Np, Mp, opt)
    walk = direct_walk(Np, Mp, opt)
    live = [w for w in walk if w is not None]
    assert len(walk) == grid and sorted((tm, tn) for tm, tn, _ in live) == [(tm, tn) for tm in range(ntmT) for tn in range(Mp // 128)]
    assert max(st for _, _, st in live) == nst - 1 and len({st for _, _, st in live}) == nst        # no empty super-tile, none beyond
    idle_inside = sum(1 for blk, w in enumerate(walk) if w is None and _slot(blk, 32)[0] < nst)
    nfull = ntmT // bh
    assert idle_inside == nst * 32 - ntmT * (Mp // 128) and idle_inside >= nfull * (per_pad - per)
    if per_pad > per:       # the padded walk: no group holds tiles of two bands, i.e. more than bh tile rows
        for st in range(nst):
            rows = {tm for tm, _, s in live if s == st}
            assert len({(ntmT - 1 - tm) // bh for tm in rows}) == 1, (name, st)
    elif name == "b":       # ... the unpadded one straddles
        assert any(len({(ntmT - 1 - tm) // bh for tm, _, s in live if s == st}) == 2 for st in range(nst))
    # heavy first: super-tile 0 starts at the last tile row
    assert walk[0][0] == ntmT - 1 and walk[0][1] == 0
    # the waves' k-ranges: wave 0 of tile row 0 is shorter than the ring of three k-tiles where ab = 1, and every nkt mod 3 occurs
    nkt = direct_wave_ktiles(Np, Mp, opt)
    assert nkt[(0, 0)] == 2 * ab and nkt[(ntmT - 1, 3)] == Np // 16 and {v % 3 for v in nkt.values()} == {0, 1, 2}
    assert ab > 1 or nkt[(0, 0)] < 3
    print(f"direct {name}: Np {Np} Mp {Mp} ab {ab} ntmT {ntmT} per {per} -> {per_pad} nst {nst} grid {grid}, {idle_inside} idle slots inside")


@pytest.mark.parametrize("N,M", list(SPLIT_CASES))
def test_split_walk_visits_every_tile_once_and_keeps_its_k_range_in_w(N, M):
    Np, Mp = padded(N), padded(M)
    wr, gsz, bh, ntmT, nst, grid = k5_split_form(Np, Mp)
    walk = split_walk(Np, Mp)
    live = [w for w in walk if w is not None]
    assert len(walk) == grid and sorted((w[0], w[1]) for w in live) == [(tm, tn) for tm in range(ntmT) for tn in range(Mp // 128)]
    assert max(w[2] for w in live) == nst - 1 and len({w[2] for w in live}) == nst
    for tm, tn, st, kcols, lock in live:
        own = (tm + 1) * 64 * wr
        assert own <= kcols <= min(own + 2048, Np), (tm, tn, st, kcols)
        assert kcols % 128 == 0                      # whole k-ranges of 8 k-tiles: the loop unrolled by 4 has no remainder
        if not lock:
            assert kcols == own
    _, want_lock, want_own = SPLIT_CASES[(N, M)]
    assert sorted({w[2] for w in live if w[4]}) == want_lock and sorted({w[2] for w in live if not w[4]}) == want_own
    extra = max(w[3] - (w[0] + 1) * 64 * wr for w in live)
    if want_lock and padded(M) // 128 < 8:
        assert extra > 0                             # a lockstep group over two bands really runs some tile past its own range
    print(f"split N {N} M {M}: wr {wr} ntmT {ntmT} nst {nst} grid {grid}: lockstep {want_lock}, own {want_own}, at most {extra} columns past the row's own range")


def _bar_case(kind, N, M, D, scale_case=False):
    X, Xq, ls, W = case_operands(N, M, D)
    if scale_case:
        W = scale_case_factor()[1]
    Np = W.shape[0]
    bar, e_full, e_cross, which = case_bar(kind, N, M, D, 0, scale_case)
    K = kstar(X, Xq[:_emu_cols(M)], ls, Np)
    S = s_reference(W, K)
    return W, K.numpy(), S, Np, bar, e_full, e_cross, which


@pytest.mark.parametrize("name", list(DIRECT_CASES))
def test_direct_bar_lies_above_the_emulation_and_under_every_fault(name):
    N, M, D, opt = DIRECT_CASES[name]
    W, K, S, Np, bar, e_full, e_cross, which = _bar_case("direct", N, M, D)
    shifts = [fault_shift(W, K, S, rb, kb) for rb, kb in fault_places(N, Np)]
    e_other = rel_err(emulate_direct(W, K, drop="a0b1"), S)
    print(f"direct {name}: Np {Np}, {K.shape[0]} queries: emulation {e_full:.2e}, without {which} {e_cross:.2e}, without a0b1 {e_other:.2e}, "
          f"faults {' '.join(f'{s:.2e}' for s in shifts)}, 128 / Np^2 {128 / Np ** 2:.2e}, bar {bar:.2e}")
    assert (which == "a0b1") == (name == "h")
    assert e_full <= bar / 8
    assert min(shifts) > 4 * bar and e_other >= 4 * bar


@pytest.mark.parametrize("N,M", list(SPLIT_CASES))
def test_split_bar_lies_above_the_emulation_and_under_every_fault(N, M):
    W, K, S, Np, bar, e_full, e_cross, which = _bar_case("split", N, M, SPLIT_D)
    shifts = [fault_shift(W, K, S, rb, kb) for rb, kb in fault_places(N, Np)]
    print(f"split N {N} M {M}: Np {Np}: emulation {e_full:.2e}, without a1b0 {e_cross:.2e}, faults {' '.join(f'{s:.2e}' for s in shifts)}, "
          f"128 / Np^2 {128 / Np ** 2:.2e}, bar {bar:.2e}")
    assert which == "a1b0" and e_full <= bar / 8 and min(shifts) > 4 * bar
    # the bf16 x 3 lockstep relies on it: W is exactly zero above the diagonal
    assert not np.triu(W, 1).any()


def test_scale_case_bar_and_scales():
    N, M, D = SCALE_CASE
    W, K, S, Np, bar, e_full, e_cross, which = _bar_case("direct", N, M, D, scale_case=True)
    W64, W32 = scale_case_factor()
    assert np.array_equal(W, W32) and Np == N
    sc = split2_scales(W32)
    for b, want in enumerate(SCALE_WANT):
        blk = W32[128 * b:128 * b + 128]
        if want is not None:
            assert sc[b] == np.float32(want), (b, sc[b])
        else:                                        # an ordinary block: the maximum lands in (2^14, 2^15]
            assert 2.0 ** 14 < float(np.abs(blk).max()) * float(sc[b]) <= 2.0 ** 15
    assert not W32[128:256].any() and not W32[640:].any() and W64[640:].any()        # zeros / rounded to zero in fp32
    assert W32[256:384].any() and float(np.abs(W32[256:384]).max()) * 2.0 ** 100 < 1.0       # clamped: far below 2^15 after scaling
    # S is the 2^40 block's: a fault there shows, and the emulation (zero blocks, clamped scales, 2^-22) is finite and accurate
    shift = fault_shift(W, K, S, 4 * 4 + 1, 3)
    print(f"scale case: emulation {e_full:.2e}, without a1b0 {e_cross:.2e}, fault in the 2^40 block {shift:.2e}, bar {bar:.2e}, scales {sc}")
    assert np.all(np.isfinite(emulate_direct(W32, K))) and e_full <= bar / 8 and shift > 4 * bar


def test_operands_are_what_the_docstring_says():
    X, Xq, ls, W = case_operands(1100, 1900, 6)
    N, Np = 1100, 1152
    assert X.dtype == np.float32 and Xq.dtype == np.float32 and W.dtype == np.float32 and W.shape == (Np, Np)
    assert not np.triu(W, 1).any() and np.count_nonzero(np.tril(W)) == Np * (Np + 1) // 2
    ssq = np.einsum("ij,ij->i", W[:, :N].astype(np.float64), W[:, :N].astype(np.float64))
    assert np.max(np.abs(ssq - 1.0)) < 1e-6
    assert case_operands(1100, 300, 6)[3] is W                       # one factor per N
    # K*: zero for j >= N, the oracle's values before
    K = kstar(X, Xq[:128], ls, Np).numpy()
    from oracle import gp_oracle as O
    want = O.rbf_cross(Xq[:128].astype(np.float64), X.astype(np.float64), ls, SF2)
    assert not K[:, N:].any() and np.max(np.abs(K[:, :N] - want)) < 1e-15 * SF2 * 8


def test_decode_split2_rows_and_parts():
    rng = np.random.default_rng(11)
    Np = 256
    KB = Np // 16
    W = np.tril(rng.standard_normal((Np, Np))).astype(np.float32)
    sc = split2_scales(W)
    assert sc.shape == (2,) and all(2.0 ** 14 < np.abs(W[128 * b:128 * b + 128]).max() * sc[b] <= 2.0 ** 15 for b in range(2))
    h0, h1 = split2_parts(W * np.repeat(sc, 128)[:, None])
    back = h0.astype(np.float64) + h1.astype(np.float64) - (W * np.repeat(sc, 128)[:, None]).astype(np.float64)
    assert np.max(np.abs(back) / np.maximum(2.0 ** -23 * np.abs(W * np.repeat(sc, 128)[:, None]), 2.0 ** -25)) <= 1.0
    raw = np.full(Np * Np * 2 + 16, np.float16(7.0), dtype=np.float16)
    for r in range(Np):
        for kb in range(KB):
            for h in range(2):
                for s, part in ((0, h0), (1, h1)):
                    chunk = (((r // 32) * KB + kb) * 2 + s) * 64 + h * 32 + r % 32
                    raw[8 * chunk:8 * chunk + 8] = part[r, 16 * kb + 8 * h:16 * kb + 8 * h + 8]
    d0, d1 = decode_split2_rows(raw.view(np.uint8), Np)
    assert np.array_equal(d0, h0.astype(np.float64)) and np.array_equal(d1, h1.astype(np.float64))
    # the scales at the edges of absmax_to_scale_kernel: an exact power of two takes 15 - e, anything above it 14 - e
    E = np.zeros((384, 384), dtype=np.float32)
    E[0, 0], E[128, 5], E[300, 300], E[10, 200] = 0.5, 0.5000001, 3.0, 1e30       # (the last lies above the diagonal: not counted)
    assert np.array_equal(split2_scales(E), np.array([2.0 ** 16, 2.0 ** 15, 2.0 ** 13], dtype=np.float32))
    # bf16 x 3: exact
    x = rng.standard_normal(4096).astype(np.float32) * np.float32(3e-5)
    x0, x1, x2 = split3_parts(x)
    assert np.array_equal((x0.astype(np.float64) + x1) + x2, x.astype(np.float64))
    assert all(not (p.view(np.uint32) & 0xffff).any() for p in (x0, x1, x2))
