"""Support shared by the test modules (a plain module: nothing here is collected): ctypes and sequence helpers, the test matrices
more than one file is built on, and Raw -- one index straight on the C ABI -- for the compaction, fold, collapse and build-columns
GPU tests.  The wrappers of the calls under test (compact, fold, insert, column) stay beside the tests that use them."""
import ctypes as C

import numpy as np


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rand_seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode("ascii")


def ragged_bits(m, n):
    """Every column distinct: column c set in exactly the rows r < (c * 37) % (m + 1), and the row r = c % m flipped, so that two
    columns with the same height still differ."""
    bits = (np.arange(m)[:, None] < ((np.arange(n) * 37) % (m + 1))[None, :]).astype(np.uint8)
    bits[np.arange(n) % m, np.arange(n)] ^= 1
    return bits


def junk_rows(rng, m, n, stride):
    """Random rows at the full stride: bits beyond column n - 1 (the rest of the last byte and the padding) are set too, and a fold
    must drop them."""
    return rng.integers(0, 256, size=(m, stride), dtype=np.uint8)


class Raw(object):
    """One index straight on the C ABI; write() stores rows at any width up to the stride with bigsi_hip_set_rows."""

    def __init__(self, m, n=0, cap=None, h=3, packed=None):
        from bigsi_amd import _lib
        self.L, self.lib = _lib.lib(), _lib
        self.ix = C.c_void_p()
        _lib.check(self.L.bigsi_hip_open(m, n, cap or max(n, 1), h, 0, C.byref(self.ix)))
        if packed is not None:
            self.write(packed)

    @classmethod
    def from_bits(cls, bits, cap=None):
        """An index holding the bit matrix `bits` (uint8[m, n] of 0 / 1)."""
        return cls(m=bits.shape[0], n=bits.shape[1], cap=cap, packed=np.packbits(bits, axis=1))

    def write(self, packed):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        ids = np.arange(packed.shape[0], dtype=np.uint64)
        self.lib.check(self.L.bigsi_hip_set_rows(self.ix, ptr(ids), ids.size, ptr(packed), packed.shape[1]))

    def info(self, handle=None):
        inf = self.lib.Info()
        self.lib.check(self.L.bigsi_hip_get_info(handle or self.ix, C.byref(inf)))
        return inf

    @property
    def stride(self):
        return int(self.info().row_stride_bytes)

    @property
    def num_cols(self):
        return int(self.info().num_cols)

    def rows(self, *, ids=None, row_bytes=None, handle=None):
        """The rows `ids` (default: every row the index says it has) at `row_bytes` bytes each (default: the whole stride), read
        through `handle` (default: the index's own) over a buffer preset to a pattern."""
        inf = self.info(handle)
        ids = np.arange(int(inf.num_rows), dtype=np.uint64) if ids is None else np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.full((ids.size, int(inf.row_stride_bytes) if row_bytes is None else row_bytes), 0xAB, np.uint8)
        self.lib.check(self.L.bigsi_hip_get_rows(handle or self.ix, ptr(ids), ids.size, ptr(out), out.shape[1]))
        return out

    def err(self):
        return self.L.bigsi_hip_last_error()

    def close(self):
        self.lib.check(self.L.bigsi_hip_close(self.ix))
