"""The build side without a GPU: the plain numpy statements of insert_columns, insert_column, get_column and the merge
(expected_insert, expected_append, expected_column) that tests/test_gpu_build_columns.py holds the kernels against, themselves
compared here with libbigsi_cpu.so -- the CPU twin, which moves one bit at a time as the reference does -- on a sweep of small shapes.
Everything is uint8 in the row byte format: column c of a row is byte c // 8 under 0x80 >> (c % 8), row r of a filter likewise."""
import ctypes as C

import numpy as np
import pytest

from raw_index import junk_rows, ptr
from test_fold_rows_host import cpu, twin_info, twin_open, twin_rows, twin_write          # noqa: F401  (cpu is a fixture)

ERR_RANGE = -4
ROW_BLOCK = 1024


# --------------------------------------------------------------------------------------------- the reference
def expected_insert(rows_packed, n_cols_before, col0, filters, m, row0=0):
    """What insert_columns leaves of rows [row0, row0 + len(rows_packed)) of an m-row index (rows_packed: those rows at any width, as
    they were): columns [col0, col0 + n) of row r become bit r of filter 0 .. n - 1 (filters: uint8[n, >= ceil(m / 8)], only the
    first m bits of each are looked at); every other bit of the row, at or behind n_cols_before too, stays as it was.  row0 is a
    multiple of 8.  ROW_BLOCK rows at a time: the bits of a block, never of the matrix, are spread out to bytes."""
    rows_packed, filters = np.asarray(rows_packed, np.uint8), np.asarray(filters, np.uint8)
    n, count = filters.shape[0], rows_packed.shape[0]
    assert col0 <= n_cols_before and row0 % 8 == 0 and row0 + count <= m and (col0 + n + 7) // 8 <= rows_packed.shape[1]
    assert filters.shape[1] * 8 >= m
    out = rows_packed.copy()
    if n == 0:
        return out
    b_lo, b_hi = col0 // 8, (col0 + n + 7) // 8          # the row bytes that hold a column of [col0, col0 + n)
    for r0 in range(0, count, ROW_BLOCK):
        r1 = min(count, r0 + ROW_BLOCK)
        f_lo, f_hi = (row0 + r0) // 8, (row0 + r1 + 7) // 8
        fbits = np.unpackbits(filters[:, f_lo:f_hi], axis=1)[:, :r1 - r0]          # [filter, row of the block]
        bits = np.unpackbits(out[r0:r1, b_lo:b_hi], axis=1)
        bits[:, col0 - 8 * b_lo:col0 - 8 * b_lo + n] = fbits.T
        out[r0:r1, b_lo:b_hi] = np.packbits(bits, axis=1)
    return out


def expected_append(dst_rows, n1, src_rows, n2, out_bytes=None):
    """The merge: columns [0, n1) of the destination's rows, then columns [0, n2) of the source's, zeros up to out_bytes (the
    destination's width by default).  Whatever the source holds behind column n2 - 1 does not come along."""
    dst_rows, src_rows = np.asarray(dst_rows, np.uint8), np.asarray(src_rows, np.uint8)
    out_bytes = dst_rows.shape[1] if out_bytes is None else out_bytes
    assert dst_rows.shape[0] == src_rows.shape[0] and (n1 + n2 + 7) // 8 <= out_bytes
    bits = np.concatenate([np.unpackbits(dst_rows, axis=1)[:, :n1], np.unpackbits(src_rows, axis=1)[:, :n2]], axis=1)
    out = np.zeros((dst_rows.shape[0], out_bytes), np.uint8)
    if n1 + n2:
        out[:, :(n1 + n2 + 7) // 8] = np.packbits(bits, axis=1)
    return out


def expected_column(rows_packed, col, m):
    """get_column: bit `col` of rows 0 .. m - 1 as one filter of ceil(m / 8) bytes; the bits of the last byte behind row m - 1 are zero."""
    rows_packed = np.asarray(rows_packed, np.uint8)
    assert rows_packed.shape[0] == m
    return np.packbits((rows_packed[:, col // 8] >> (7 - col % 8)) & 1)


def clean_rows(rng, m, n, stride):
    """Random columns [0, n), zeros behind them up to the stride: the library's own invariant for an index of n columns."""
    return expected_append(np.zeros((m, stride), np.uint8), 0, junk_rows(rng, m, n, (n + 7) // 8 or 1), n)


def junk_filters(rng, n, m, pitch=None):
    """n random filters of m bits at a pitch of at least ceil(m / 8) bytes; the bits of the last byte behind row m - 1 and the bytes
    up to the pitch are random too: none of them may reach a row."""
    return rng.integers(0, 256, size=(n, pitch or (m + 7) // 8), dtype=np.uint8)


# --------------------------------------------------------------------------------------------- the reference against itself
def test_expected_insert_bit_by_bit():
    """expected_insert against the definition spelled out one bit at a time, on shapes that cross a row block and a byte both ways;
    with row0 it gives the same rows as the slice of the whole."""
    rng = np.random.default_rng(1)
    for m, n0, col0, n in ((1, 0, 0, 1), (9, 13, 5, 3), (1030, 20, 20, 9), (2049, 40, 7, 30), (1025, 0, 0, 17)):
        stride = 16
        rows, filters = junk_rows(rng, m, n0, stride), junk_filters(rng, n, m, (m + 7) // 8 + 3)
        want = np.unpackbits(rows, axis=1)
        for c in range(n):
            for r in range(m):
                want[r, col0 + c] = (filters[c, r // 8] >> (7 - r % 8)) & 1
        got = expected_insert(rows, n0, col0, filters, m)
        assert np.array_equal(got, np.packbits(want, axis=1)), (m, n0, col0, n)
        if m > 16:
            r0 = (m // 2) // 8 * 8
            assert np.array_equal(expected_insert(rows[r0:], n0, col0, filters, m, row0=r0), got[r0:])
            assert np.array_equal(expected_insert(rows[8:16], n0, col0, filters, m, row0=8), got[8:16])


# --------------------------------------------------------------------------------------------- against the CPU twin
def twin_insert(L, ix, col0, filters):
    filters = np.ascontiguousarray(filters)
    return L.bigsi_cpu_insert_columns(ix, C.c_uint64(col0), C.c_uint64(filters.shape[0]), ptr(filters), C.c_uint64(filters.shape[1]))


def twin_column(L, ix, col, m):
    out = np.full((m + 7) // 8, 0xAB, np.uint8)
    rc = L.bigsi_cpu_get_column(ix, C.c_uint64(col), ptr(out))
    return rc, out


@pytest.mark.parametrize("m", [1, 7, 8, 9, 63, 65, 130])
def test_insert_columns_against_the_twin(cpu, m):
    """Overwrites inside a junk-filled index (every bit outside [col0, col0 + n) stays, behind num_cols too) and appends to a clean one,
    at column offsets and counts on both sides of a byte and of a 64-column word; filters at a pitch with junk behind their m bits."""
    rng = np.random.default_rng(m)
    for n0, col0, n in ((0, 0, 1), (0, 0, 64), (0, 0, 130), (1, 1, 63), (5, 5, 3), (64, 64, 1), (63, 60, 10), (100, 0, 99), (100, 7, 57), (100, 64, 36),
                        (100, 100, 29), (129, 127, 2), (129, 128, 1), (200, 8, 64), (200, 63, 66), (200, 200, 56)):
        ix = twin_open(cpu, m, n0, cap=256)
        stride = int(twin_info(cpu, ix).row_stride_bytes)
        inside = col0 + n < n0
        rows = junk_rows(rng, m, n0, stride) if inside else clean_rows(rng, m, n0, stride)
        twin_write(cpu, ix, rows)
        filters = junk_filters(rng, n, m, (m + 7) // 8 + int(rng.integers(0, 5)))
        assert twin_insert(cpu, ix, col0, filters) == 0, cpu.bigsi_cpu_last_error()
        assert twin_info(cpu, ix).num_cols == max(n0, col0 + n)
        assert np.array_equal(twin_rows(cpu, ix, m, stride), expected_insert(rows, n0, col0, filters, m)), (m, n0, col0, n)
        assert cpu.bigsi_cpu_close(ix) == 0


@pytest.mark.parametrize("m", [1, 9, 63, 130])
def test_insert_column_and_get_column_against_the_twin(cpu, m):
    """One column at a time: overwrites at 0, 7, 8, 63, 64 and the append at num_cols, into rows of junk; get_column of every column the
    index has reads what expected_column says, pad bits zero; a column at or behind num_cols is refused and the buffer left alone."""
    rng = np.random.default_rng(100 + m)
    n0 = 100
    ix = twin_open(cpu, m, n0, cap=256)
    stride = int(twin_info(cpu, ix).row_stride_bytes)
    rows = junk_rows(rng, m, n0, stride)
    twin_write(cpu, ix, rows)
    for col in (0, 7, 8, 63, 64, n0):
        bloom = junk_filters(rng, 1, m)
        assert cpu.bigsi_cpu_insert_column(ix, C.c_uint64(col), ptr(bloom)) == 0, cpu.bigsi_cpu_last_error()
        rows = expected_insert(rows, n0, col, bloom, m)
        assert np.array_equal(twin_rows(cpu, ix, m, stride), rows), (m, col)
    assert twin_info(cpu, ix).num_cols == n0 + 1
    for col in range(n0 + 1):
        rc, got = twin_column(cpu, ix, col, m)
        assert rc == 0 and np.array_equal(got, expected_column(rows, col, m)), (m, col)
    for col in (n0 + 1, n0 + 2, stride * 8 - 1, stride * 8):
        rc, got = twin_column(cpu, ix, col, m)
        assert rc == ERR_RANGE and (got == 0xAB).all(), (m, col)
    assert cpu.bigsi_cpu_close(ix) == 0


def twin_append(L, dst, src, m):
    """The merge as the twin can do it: room in the destination, then every column of the source read with get_column and appended with
    insert_column -- one bit at a time, both ways."""
    n1, n2 = int(twin_info(L, dst).num_cols), int(twin_info(L, src).num_cols)
    assert L.bigsi_cpu_reserve_cols(dst, C.c_uint64(n1 + n2)) == 0, L.bigsi_cpu_last_error()
    for j in range(n2):
        rc, col = twin_column(L, src, j, m)
        assert rc == 0
        assert L.bigsi_cpu_insert_column(dst, C.c_uint64(n1 + j), ptr(col)) == 0, L.bigsi_cpu_last_error()


@pytest.mark.parametrize("junk", [False, True])
def test_append_against_the_twin(cpu, junk):
    """expected_append against the twin's column-by-column merge, for a source that is clean behind its columns and for one whose
    whole stride is junk: the same destination either way, re-strided where n1 + n2 outgrows it."""
    m = 37
    rng = np.random.default_rng(7 + junk)
    for n1, n2 in ((0, 1), (0, 70), (1, 63), (1, 64), (63, 1), (63, 65), (64, 64), (65, 64), (127, 65), (128, 129), (200, 63), (200, 900), (1000, 100)):
        dst, src = twin_open(cpu, m, n1), twin_open(cpu, m, n2, cap=n2 + 700)
        d_stride, s_stride = int(twin_info(cpu, dst).row_stride_bytes), int(twin_info(cpu, src).row_stride_bytes)
        d_rows = clean_rows(rng, m, n1, d_stride)
        s_rows = junk_rows(rng, m, n2, s_stride) if junk else clean_rows(rng, m, n2, s_stride)
        twin_write(cpu, dst, d_rows)
        twin_write(cpu, src, s_rows)
        twin_append(cpu, dst, src, m)
        inf = twin_info(cpu, dst)
        assert inf.num_cols == n1 + n2 and (int(inf.row_stride_bytes) > d_stride) == (n1 + n2 > d_stride * 8)
        assert np.array_equal(twin_rows(cpu, dst, m, int(inf.row_stride_bytes)), expected_append(d_rows, n1, s_rows, n2, int(inf.row_stride_bytes))), (n1, n2)
        assert np.array_equal(twin_rows(cpu, src, m, s_stride), s_rows)
        for h in (dst, src):
            assert cpu.bigsi_cpu_close(h) == 0
