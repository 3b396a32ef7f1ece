"""The build side on the device -- bigsi_hip_insert_columns / bigsi_hip_insert_columns_device (k_transpose_regs for whole tiles,
k_insert_columns for ragged heads and tails), bigsi_hip_append_index (k_append_columns), bigsi_hip_insert_column / get_column --
bit for bit against the numpy statements of tests/test_build_columns_host.py, which that file holds against the CPU twin.  Filters
are seeded random bytes (density 0.5), not hashed k-mers; rows go in with set_rows and come back with get_rows at the WHOLE stride
over a buffer preset to a pattern; every comparison is np.array_equal on packed bytes.

Two invariants, for every insert below:
  OVERWRITE inside the index (col0 + n < num_cols): every bit outside [col0, col0 + n) keeps its value -- the bits behind num_cols
    too, so the index is filled with random bytes over its whole stride first;
  APPEND (col0 + n >= num_cols): the index is zero behind num_cols beforehand (the library's own invariant); afterwards the columns
    below col0 are unchanged, [col0, end) are the filters, and everything from `end` to the end of the stride reads back as zero --
    the tiled kernel writes whole 128-byte lines there, zeros for the columns that have no filter.

The geometry the cases rest on (transpose_device, k_transpose_regs<2>): a tile is 1024 rows x 16 words (1024 columns); the tiled path
starts at round_up(col0, 128); sup_w = the power of two >= tiles_c, at most 32; a supertile is sup_w x (1024 / sup_w) tiles; XCD
groups are 4 tile rows x 1 tile column.

What results cannot see, here or anywhere: the `+ 4` of the LDS pitch and the `& 8` of its swizzle (any one-to-one map of the image's
words gives the same rows: they only keep LDS banks apart), and the guards `off < nb` of the tiled loads and `q < src_words` of the
merge (what they keep from being loaded belongs to rows >= num_rows or to columns >= n1 + n2 and is never stored: they only keep the
loads inside the caller's bytes)."""
import ctypes as C
import time

import numpy as np
import pytest

from raw_index import Raw, junk_rows, ptr
from test_build_columns_host import clean_rows, expected_append, expected_column, expected_insert, junk_filters

pytestmark = pytest.mark.gpu
ERR_RANGE, ERR_CAPACITY = -4, -5


def insert(a, col0, filters):
    filters = np.ascontiguousarray(filters, dtype=np.uint8)
    return a.L.bigsi_hip_insert_columns(a.ix, col0, filters.shape[0], ptr(filters), filters.shape[1])


def insert_column(a, col, bloom):
    return a.L.bigsi_hip_insert_column(a.ix, col, ptr(np.ascontiguousarray(bloom, dtype=np.uint8)))


def column(a, col):
    out = np.full((int(a.info().num_rows) + 7) // 8, 0xAB, np.uint8)
    return a.L.bigsi_hip_get_column(a.ix, col, ptr(out)), out


def check_append(m, n0, n, cap, seed, pitch_extra=0):
    """APPEND: n filters at col0 = n0 into an index of n0 random columns, clean behind them."""
    rng = np.random.default_rng(seed)
    a = Raw(m, n0, cap or n0 + n)
    try:
        before = clean_rows(rng, m, n0, a.stride)
        if n0:
            a.write(before)
        filters = junk_filters(rng, n, m, (m + 7) // 8 + pitch_extra)
        assert insert(a, n0, filters) == 0, a.err()
        assert a.num_cols == n0 + n and a.stride == before.shape[1]
        assert np.array_equal(a.rows(), expected_insert(before, n0, n0, filters, m)), (m, n0, n)
    finally:
        a.close()


# --------------------------------------------------------------------------------------------- (a) tile edges
# (m, n) at col0 = 0 into an empty index.  Between them every m of {1, 7, 8, 9, 127, 129, 511, 513, 1023, 1024, 1025, 2049, 4100}: both sides
# of a byte, of a thread's 16-byte load (128 rows), of a 512-row half, of a tile, and m > 4096 = more than one XCD group of 4 tile rows;
# every n of {127, 128, 129, 191, 192, 1023, 1024, 1025, 1151, 2048, 2049, 3000, 4100}: both sides of a word, of the 128-column threshold of
# the tiled path and of a tile; tiles_c = 1, 2, 3, 5, so sup_w = 1, 2, 4, 8.  The extremes of m meet the extremes of n.
TILE_EDGES = [(1, 127), (1, 4100), (4100, 127), (4100, 4100), (7, 128), (8, 129), (9, 191), (127, 192), (129, 1023), (511, 1024), (513, 1025),
              (1023, 1151), (1024, 2048), (1025, 2049), (2049, 3000), (1024, 1025), (2049, 128), (4100, 1024), (1025, 3000)]


@pytest.mark.parametrize("i", range(len(TILE_EDGES)))
def test_a_tile_edges(i):
    m, n = TILE_EDGES[i]
    check_append(m, 0, n, n + (5000 if i % 2 else 0), 1000 + i, pitch_extra=i % 3)


# --------------------------------------------------------------------------------------------- (b), (c) the supertile decode
def test_b_full_supertile_decode():
    """tiles_c = 18: sup_w = 32, two supertile rows (33 tile rows of 1024), every one of the 256 groups of the first supertile used,
    and most workgroups of the second return early.  72 MB of filters, 78 MB of matrix."""
    t0 = time.perf_counter()
    check_append(32768 + 1000 + 5, 0, 17 * 1024 + 300, None, 2000)
    print("test_b wall time: %.2f s" % (time.perf_counter() - t0))


def test_c_two_supertiles_along_the_columns():
    """tiles_c = 34: sup_c = 2, the second supertile column holds tile columns 32 and 33."""
    check_append(1100, 0, 33 * 1024 + 100, None, 3000)


# --------------------------------------------------------------------------------------------- (d) heads, tails, the capacity clamp
M_D = 1025


@pytest.mark.parametrize("n0", [1, 64, 100, 127, 128, 129, 200])
def test_d_ragged_head_then_tiles(n0):
    check_append(M_D, n0, 1300, n0 + 1300, 4000 + n0)


@pytest.mark.parametrize("col0,n", [(5, 3), (5, 200), (100, 1024), (128, 1024), (129, 1100), (1000, 64), (0, 2999)])
def test_d_overwrite_strictly_inside(col0, n):
    """OVERWRITE: the tiled kernel takes whole words only, the tail goes column by column, and nothing else moves."""
    rng = np.random.default_rng(5000 + col0)
    a = Raw(M_D, 3000, 3000 + (2000 if col0 % 2 else 0))
    try:
        before = junk_rows(rng, M_D, 3000, a.stride)
        a.write(before)
        filters = junk_filters(rng, n, M_D, 144)
        assert insert(a, col0, filters) == 0, a.err()
        assert a.num_cols == 3000
        assert np.array_equal(a.rows(), expected_insert(before, 3000, col0, filters, M_D)), (col0, n)
    finally:
        a.close()


@pytest.mark.parametrize("n0,cap,col0,n", [(3000, 3000, 129, 2871), (3000, 5000, 2900, 100),          # end == num_cols exactly
                                           (100, 1024, 100, 924),                                      # n_words clamped to 14 by the stride of 16
                                           (1023, 1024, 1023, 1), (1024, 1024, 1023, 1)])             # the last column of the capacity
def test_d_up_to_num_cols_and_capacity(n0, cap, col0, n):
    rng = np.random.default_rng(6000 + col0 + n0)
    a = Raw(M_D, n0, cap)
    try:
        assert a.stride == (cap + 1023) // 1024 * 128
        before = clean_rows(rng, M_D, n0, a.stride)
        a.write(before)
        filters = junk_filters(rng, n, M_D, 256)
        assert insert(a, col0, filters) == 0, a.err()
        assert a.num_cols == max(n0, col0 + n)
        want = expected_insert(before, n0, col0, filters, M_D)
        assert np.array_equal(a.rows(), want), (n0, cap, col0, n)
        if col0 + 1 + n > a.stride * 8:          # one column further is refused, and nothing written
            assert insert(a, col0 + 1, filters) == ERR_CAPACITY and np.array_equal(a.rows(), want)
    finally:
        a.close()


# --------------------------------------------------------------------------------------------- (e) the device entry
M_E, N_E, N0_E = 1025 + 4, 1500, 3
NB_E = (M_E + 7) // 8          # 129


@pytest.mark.parametrize("pitch,offset", [(144, 0), (256, 0), (144 + 48, 0), (144, 16), (144, 8), (NB_E, 0)],
                         ids=["pitch16", "pitch128", "pitch16+48", "pointer+16", "pointer+8_slow", "odd_pitch_slow"])
def test_e_device_entry(pitch, offset):
    """Filters resident in device memory at the caller's pitch and pointer.  The whole buffer is 0xFF before the filters go in and the
    bits of byte nb - 1 behind row m - 1 are set, so every pad byte and pad bit is junk; the reference looks at the first m bits only."""
    import torch
    rng = np.random.default_rng(7000)          # the same filters and index for every variant: the same rows
    a = Raw(M_E, N0_E, N0_E + N_E)
    try:
        before = clean_rows(rng, M_E, N0_E, a.stride)
        a.write(before)
        filters = junk_filters(rng, N_E, M_E)
        filters[:, NB_E - 1] |= 0xFF >> (M_E - 8 * (NB_E - 1))
        host = np.full(offset + N_E * pitch, 0xFF, np.uint8)
        host[offset:].reshape(N_E, pitch)[:, :NB_E] = filters
        dev = torch.from_numpy(host).to("cuda")
        torch.cuda.synchronize()
        assert dev.data_ptr() % 16 == 0
        assert a.L.bigsi_hip_insert_columns_device(a.ix, N0_E, N_E, dev.data_ptr() + offset, pitch) == 0, a.err()
        assert a.num_cols == N0_E + N_E
        assert np.array_equal(a.rows(), expected_insert(before, N0_E, N0_E, filters, M_E))
        assert np.array_equal(dev.cpu().numpy(), host)          # the filters are only read
    finally:
        a.close()


# --------------------------------------------------------------------------------------------- (f) the slab loop, the 4 KB pitch rule
def test_f_three_slabs_at_two_million_rows():
    """m = 2^21: a filter is 256 KB, a multiple of 4 KB, so the staging pitch is 262144 + 128 and a 256 MB slab holds 896 filters: 2100
    filters behind 40 existing columns go in as slabs at columns 40, 936 and 1832, each with a ragged head.  Three blocks of 1024
    full-stride rows (the first, one across row 2^20, the last) against numpy, and ten columns over all rows through get_column."""
    t0 = time.perf_counter()
    m, n0, n = 1 << 21, 40, 2100
    nb = m // 8
    rng = np.random.default_rng(8000)
    block = rng.integers(0, 256, size=(256, nb), dtype=np.uint8)          # 64 MB of random bytes, repeated under a XOR byte of each repeat's own
    filters = np.empty((n, nb), np.uint8)
    for j in range(0, n, 256):
        np.bitwise_xor(block[:min(256, n - j)], np.uint8((j // 256) * 29), out=filters[j:j + 256])
    head = rng.integers(0, 256, size=(m, n0 // 8), dtype=np.uint8)          # the 40 columns there are: set_rows zeroes the rest of the stride
    a = Raw(m, n0, n0 + n)
    try:
        a.write(head)
        stride = a.stride
        assert stride == 384
        assert insert(a, n0, filters) == 0, a.err()
        assert a.num_cols == n0 + n
        for r0 in (0, (1 << 20) - 512, m - 1024):
            before = np.zeros((1024, stride), np.uint8)
            before[:, :n0 // 8] = head[r0:r0 + 1024]
            got = a.rows(ids=np.arange(r0, r0 + 1024))
            assert np.array_equal(got, expected_insert(before, n0, n0, filters, m, row0=r0)), r0
        for col in (0, 39, 40, 935, 936, 1023, 1024, 1831, 1832, 2139):
            rc, got = column(a, col)
            want = filters[col - n0] if col >= n0 else np.packbits((head[:, col // 8] >> (7 - col % 8)) & 1)
            assert rc == 0 and np.array_equal(got, want), col
    finally:
        a.close()
    print("test_f wall time: %.2f s" % (time.perf_counter() - t0))


# --------------------------------------------------------------------------------------------- (g) the merge
# (n1, n2): n1 % 64 == 0 -- (0, 1000), (64, 64), (128, 129), (128, 1000); (n1 + n2) % 64 == 0 -- (1, 63), (63, 1), (63, 65), (64, 64), (127, 65);
# more destination words than source words -- (1, 64), (65, 64), (200, 63), (63, 1000); n1 + n2 beyond the destination's 1024 columns, so
# that reserve_cols re-strides -- (63, 1000), (128, 1000), (200, 1000)
APPENDS = [(0, 1000), (1, 63), (1, 64), (63, 1), (63, 65), (63, 1000), (64, 64), (65, 64), (127, 65), (128, 129), (128, 1000), (200, 63), (200, 1000), (64, 129)]
M_G = 257


@pytest.mark.parametrize("junk", [False, True], ids=["clean_source", "junk_behind_source"])
@pytest.mark.parametrize("i", range(len(APPENDS)))
def test_g_append_index(i, junk):
    """junk: the source's rows hold random bits behind its n2 columns over its whole stride (set_rows can put them there); none of
    them may reach the destination, whose stride behind n1 + n2 is zero."""
    n1, n2 = APPENDS[i]
    rng = np.random.default_rng(9000 + i)
    dst, src = Raw(M_G, n1), Raw(M_G, n2, n2 + (3000 if i % 2 else 0))
    try:
        d_rows = clean_rows(rng, M_G, n1, dst.stride)
        s_rows = clean_rows(rng, M_G, n2, src.stride)
        if junk:
            behind = junk_rows(rng, M_G, 0, src.stride)
            s_rows[:, n2 // 8 + 1:] = behind[:, n2 // 8 + 1:]
            s_rows[:, n2 // 8] |= behind[:, n2 // 8] & (0xFF >> (n2 % 8))
        if n1:
            dst.write(d_rows)
        src.write(s_rows)
        assert dst.stride == 128
        assert dst.L.bigsi_hip_append_index(dst.ix, src.ix) == 0, dst.err()
        assert dst.num_cols == n1 + n2 and dst.stride == (n1 + n2 + 1023) // 1024 * 128
        assert np.array_equal(dst.rows(), expected_append(d_rows, n1, s_rows, n2, dst.stride)), (n1, n2, junk)
        assert np.array_equal(src.rows(), s_rows) and src.num_cols == n2          # the source is only read
    finally:
        dst.close()
        src.close()


# --------------------------------------------------------------------------------------------- (h) one column at a time
@pytest.mark.parametrize("m", [1, 9, 1025])
def test_h_insert_column_and_get_column(m):
    """Overwrites at columns 0, 7, 8, 63, 64 and the append at num_cols, into an index whose whole stride is random: no other bit
    moves.  get_column of every column the index has, pad bits of the last byte zero; a column at or behind num_cols is refused
    (BIGSI_ERR_RANGE, the buffer left alone), as the CPU twin refuses it -- up to the capacity and beyond."""
    rng = np.random.default_rng(10000 + m)
    n0 = 100
    a = Raw(m, n0, n0)
    try:
        rows = junk_rows(rng, m, n0, a.stride)
        a.write(rows)
        for col in (0, 7, 8, 63, 64, n0):
            bloom = junk_filters(rng, 1, m)          # (the bits of its last byte behind row m - 1 are random)
            assert insert_column(a, col, bloom) == 0, a.err()
            rows = expected_insert(rows, n0, col, bloom, m)
            assert np.array_equal(a.rows(), rows), (m, col)
        assert a.num_cols == n0 + 1
        for col in range(n0 + 1):
            rc, got = column(a, col)
            assert rc == 0 and np.array_equal(got, expected_column(rows, col, m)), (m, col)
        for col in (n0 + 1, n0 + 2, 1023, 1024, 1 << 40):
            rc, got = column(a, col)
            assert rc == ERR_RANGE and (got == 0xAB).all(), (m, col)
        assert insert_column(a, n0 + 2, junk_filters(rng, 1, m)) == ERR_RANGE          # a gap is refused
        assert np.array_equal(a.rows(), rows)
    finally:
        a.close()
