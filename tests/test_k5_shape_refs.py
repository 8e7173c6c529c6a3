"""The operand addressing of the 16x16x32 form of the fp16 x 2 variance launch (k5_direct_kernel<AB, 2>, gpk_k5split.hip), restated
and checked against the fragment order without a GPU.

The form reads the operands that the 32x32x16 form reads - gpk_split2_rows' fragment order, `decode_split2_rows` - but takes a
different cut through them: lane l = 16 q + r of a wave load wants, for the 16-row group g of a 32-row block, the 32-step j and
the part s, the 16-byte chunk (row 16 g + r, k16 block 2 j + (q >> 1), half q & 1, part s) - the eight k of octet q of the step -
and finds it at byte

    4096 j + 2048 (q >> 1) + 1024 s + 512 (q & 1) + 16 (16 g + r)

of the block's strip (Np / 16 k16 blocks of 2048 bytes).  `lane_offset` is the lane's constant, `load_offset` the whole sum.

Checked here, for Np = 128 and 640 on 128-row tiles and for Np = 512 on 256- and 512-row tiles (`test_k5_refs.direct_wave_ktiles`
gives every wave's k-range, nkt k16 steps = nkt / 2 steps of 32; a wave owns the AB 32-row blocks from 4 AB tm + AB wave on):
* the 64 lanes of every (row block, row group, 32-step, part) address the eight values (row 16 g + (l & 15), k = 32 j + 8 (l >> 4) ..
  + 7) of that part, by `decode_split2_rows`' own layout (the address of every value is read back through the decoder);
* over a wave's steps every chunk of its row blocks and its k-range is addressed exactly once, and nothing else;
* no chunk lies beyond the columns that the fp64-source splitters write, 128 (row block / 4 + 1): the rest is poisoned in the GPU
  tests and, past the last row block, outside the allocation;
* the prefetches - W one step ahead, K* two steps ahead, clamped to the wave's last step - stay inside the same set;
* a wave load touches four runs of 256 bytes, eight whole 128-byte lines.

NumPy only."""
import numpy as np
import pytest

from test_k5_refs import decode_split2_rows, direct_wave_ktiles

LANES = np.arange(64)


def lane_offset(lane):
    """The lane's constant: k octet q = lane >> 4 of the 32-step, row r = lane & 15 of the 16-row group."""
    q, r = lane >> 4, lane & 15
    return (q >> 1) * 2048 + (q & 1) * 512 + r * 16


def load_offset(lane, g, j, s):
    """Byte of the chunk that `lane` loads for 16-row group g (0, 1), 32-step j and part s, inside the 32-row block's strip."""
    return 4096 * j + 1024 * s + 256 * g + lane_offset(lane)


def prefetch_step(step, nj):
    """The 32-step a prefetch of `step` really loads in a wave of nj steps (rsrc_at): past the range, the wave's last step again."""
    return min(step, nj - 1)


@pytest.fixture(scope="module", params=[128, 640, 512])
def addresses(request):
    """(Np, addr): addr[s][row, k] = index of the fp16 value (part s, row, k) in the operand, read through `decode_split2_rows`
    from an operand whose every value holds its own index (in two digits base 2048: exact in fp16)."""
    Np = request.param
    idx = np.arange(Np * Np * 2)
    lo = decode_split2_rows((idx % 2048).astype(np.float16).view(np.uint8), Np)
    hi = decode_split2_rows((idx // 2048).astype(np.float16).view(np.uint8), Np)
    assert Np * Np * 2 // 2048 < 2048
    addr = [(h * 2048 + l).astype(np.int64) for l, h in zip(lo, hi)]
    assert sorted(np.concatenate([a.ravel() for a in addr]).tolist()) == idx.tolist()
    return Np, addr


def test_lanes_address_their_rows_and_k_octets(addresses):
    Np, addr = addresses
    strip = Np // 16 * 2048
    q, r = LANES >> 4, LANES & 15
    for rb in range(Np // 32):
        for g in range(2):
            for j in range(Np // 32):
                for s in range(2):
                    off = rb * strip + load_offset(LANES, g, j, s)
                    assert np.all(off % 16 == 0)
                    got = off[:, None] // 2 + np.arange(8)[None, :]                       # the eight fp16 of each lane's chunk
                    want = addr[s][(32 * rb + 16 * g + r)[:, None], (32 * j + 8 * q)[:, None] + np.arange(8)[None, :]]
                    assert np.array_equal(got, want), (Np, rb, g, j, s)
                    # four runs of 256 bytes = eight whole cache lines
                    assert np.array_equal(np.unique(off // 128), (np.unique(off // 128)[0] + np.array([0, 1, 4, 5, 16, 17, 20, 21])))
                    assert off.min() % 256 == 0


def _tile_options(Np):
    return {128: [1], 640: [1], 512: [3, 2]}[Np]          # option k5_split2_tile: 128-row tiles; 256- and 512-row tiles


def test_a_wave_addresses_every_chunk_of_its_k_range_once_and_no_unwritten_one(addresses):
    Np, addr = addresses
    KB, strip = Np // 16, Np // 16 * 2048
    for opt in _tile_options(Np):
        nkts = direct_wave_ktiles(Np, 128, opt)
        ab = {1: 1, 3: 2, 2: 4}[opt]
        assert len(nkts) == Np // (128 * ab) * 4
        for (tm, wave), nkt in nkts.items():
            assert nkt % 2 == 0 and nkt >= 2
            nj = nkt // 2
            for a in range(ab):
                rb = 4 * ab * tm + ab * wave + a
                seen = np.concatenate([rb * strip + load_offset(LANES, g, j, s) for g in range(2) for j in range(nj) for s in range(2)]) // 16
                # chunk index (((rb KB + kb) 2 + s) 64 + h 32 + row % 32): all of kb < nkt, each once, nothing else
                want = (rb * KB * 128) + np.arange(nkt * 128)
                assert np.array_equal(np.sort(seen), want), (Np, opt, tm, wave, a)
                assert 16 * nkt <= 128 * (rb // 4 + 1) <= Np, "a chunk beyond the columns the fp64-source splitters write"
            # the prefetches: while step js runs, W of step js + 1 and K* of step js + 2, each through `prefetch_step`: every
            # chunk they address is one of the row block's own steps (`want`), also from the last two steps
            for a in range(ab):
                rb = 4 * ab * tm + ab * wave + a
                want = set(((rb * KB * 128) + np.arange(nkt * 128)).tolist())
                for js in range(nj):
                    for ahead in (1, 2):
                        pre = np.concatenate([rb * strip + load_offset(LANES, g, prefetch_step(js + ahead, nj), s) for g in range(2) for s in range(2)]) // 16
                        assert set(pre.tolist()) <= want, (Np, opt, tm, wave, a, js, ahead)
            assert prefetch_step(nj, nj) == prefetch_step(nj + 1, nj) == nj - 1 and (nj < 2 or prefetch_step(nj - 2, nj) == nj - 2)
            # K* rows (the tile's 128 queries) over the same steps: within the Np columns every row of K* has
            assert 4096 * (nj - 1) + load_offset(63, 1, 0, 1) + 16 <= strip


def test_offsets_are_the_formula_of_the_issue():
    # byte (2 j) 2048 + (q >> 1) 2048 + s 1024 + (q & 1) 512 + (16 g + r) 16
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):
        q, r = lane >> 4, lane & 15
        for g in range(2):
            for j in (0, 1, 7):
                for s in range(2):
                    assert load_offset(lane, g, j, s) == (2 * j) * 2048 + (q >> 1) * 2048 + s * 1024 + (q & 1) * 512 + (16 * g + r) * 16
    assert max(lane_offset(LANES)) + 256 + 1024 + 16 == 4096      # a step's loads end with the step's two k16 blocks
