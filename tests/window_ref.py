"""The numpy reference of the windowed search (a plain module: nothing here is collected), shared by tests/test_window_host.py and
tests/test_gpu_window.py.  Everything is computed from the bytes a test wrote into the index and the oracle's row ids: the presence of
every (position, column), its cumulative sum per column, the window differences, their maximum and first argmax, the first and last
passing start and the number of passing starts."""
import math

import numpy as np

RECORD_DTYPE = np.dtype([("best_found", np.uint32), ("best_start", np.uint32), ("first_start", np.uint32), ("last_start", np.uint32),
                         ("windows_passing", np.uint32), ("reserved", np.uint32)])
SENTINEL = 0xDEADBEEF


def presence_from_rows(rows, ids, n_cols):
    """bool[n, n_cols]: position p holds column c iff every one of the rows ids[p] (uint8 rows in the row format, at any stride) has
    bit c; the bytes and bits behind column n_cols - 1 are dropped."""
    if len(ids) == 0:
        return np.zeros((0, n_cols), bool)
    rb = (n_cols + 7) // 8
    a = np.bitwise_and.reduce(rows[np.asarray(ids, np.int64)][:, :, :rb], axis=1)
    return np.unpackbits(a, axis=1)[:, :n_cols].astype(bool)


def found_matrix(pres, window):
    """(We, found int64[n - We + 1, cols]) of a sequence's presence matrix; n == 0: (0, None)."""
    n = pres.shape[0]
    if n == 0:
        return 0, None
    we = min(window, n)
    cs = np.zeros((n + 1, pres.shape[1]), np.int64)
    cs[1:] = np.cumsum(pres, axis=0)
    return we, cs[we:] - cs[:n - we + 1]


def window_reference(pres_list, window, threshold):
    """What bigsi_hip_window_search must return for sequences with the presence matrices `pres_list`:
    (window_used uint32[n], need uint32[n], hit_offsets uint64[n + 1], colours uint32[hits], records RECORD_DTYPE[hits])."""
    used, need, off, cols, recs = [], [], [0], [], []
    for pres in pres_list:
        we, found = found_matrix(pres, window)
        nd = int(math.ceil(we * threshold))
        used.append(we)
        need.append(nd)
        if found is not None:
            ok = found >= nd
            hit = np.flatnonzero(ok.any(axis=0))
            r = np.zeros(hit.size, RECORD_DTYPE)
            r["best_found"] = found.max(axis=0)[hit]
            r["best_start"] = found.argmax(axis=0)[hit]                     # (the first maximum)
            r["first_start"] = ok.argmax(axis=0)[hit]
            r["last_start"] = found.shape[0] - 1 - ok[::-1].argmax(axis=0)[hit]
            r["windows_passing"] = ok.sum(axis=0)[hit]
            cols.append(hit.astype(np.uint32))
            recs.append(r)
        off.append(off[-1] + (len(cols[-1]) if found is not None else 0))
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)      # noqa: E731
    return np.asarray(used, np.uint32), np.asarray(need, np.uint32), np.asarray(off, np.uint64), cat(cols, np.uint32), cat(recs, RECORD_DTYPE)


class Outputs(object):
    """The output arrays of one call, sentinels behind every capacity."""

    def __init__(self, n_seqs, capacity):
        self.used = np.full(n_seqs + 2, SENTINEL, np.uint32)
        self.need = np.full(n_seqs + 2, SENTINEL, np.uint32)
        self.off = np.full(n_seqs + 3, SENTINEL, np.uint64)
        self.cols = np.full(capacity + 2, SENTINEL, np.uint32)
        self.recs = np.zeros(capacity + 2, RECORD_DTYPE)
        self.recs.view(np.uint32)[:] = SENTINEL
        self.n_seqs, self.capacity = n_seqs, capacity

    def lists_untouched(self):
        return bool((self.cols == SENTINEL).all() and (self.recs.view(np.uint32) == SENTINEL).all())

    def assert_equal(self, want):
        used, need, off, cols, recs = want
        n, total = self.n_seqs, int(off[-1])
        assert np.array_equal(self.used[:n], used) and (self.used[n:] == SENTINEL).all()
        assert np.array_equal(self.need[:n], need) and (self.need[n:] == SENTINEL).all()
        assert np.array_equal(self.off[:n + 1], off) and (self.off[n + 1:] == SENTINEL).all()
        assert np.array_equal(self.cols[:total], cols) and (self.cols[total:] == SENTINEL).all()
        for name in RECORD_DTYPE.names:
            assert np.array_equal(self.recs[name][:total], recs[name]), name
        assert (self.recs.view(np.uint32).reshape(-1, 6)[total:] == SENTINEL).all()
