"""Windowed search on the device: bigsi_hip_window_search / bigsi_hip_batch_window_search straight on the C ABI, bit-exact against the
numpy reference of tests/window_ref.py on a seeded matrix written with bigsi_hip_set_rows (m = 4096 rows, row ids from the oracle's
hashing, junk bits behind num_cols in every row, sentinels behind every output's capacity, segments forced to 64 window starts through
bigsi_hip_window_set_limits unless a case says otherwise), then BIGSI.search_windows and the `window_search` command on an index built
from sequences.  Chosen presence patterns are planted by clearing a column everywhere and setting it in all h rows of chosen positions;
every expectation is then taken from the bytes, so rows shared between positions cannot matter.  Every call that returns 0 has also
passed the library's own comparison of its two device routes (k_window_max against k_window_locate)."""
import csv
import ctypes as C
import io
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import ROOT
from raw_index import ptr, rand_seq
from oracle import coracle
from window_ref import SENTINEL, Outputs, found_matrix, presence_from_rows, window_reference

pytestmark = pytest.mark.gpu
_counter = itertools.count()
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
K, M, SEG = 31, 4096, 64


def pack(seqs):
    data = [s.encode("ascii") for s in seqs]
    off = np.zeros(len(data) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in data])
    return b"".join(data), off


def stride_of(n_cols):
    return max(128, -(-(-(-n_cols // 64) * 8) // 128) * 128)


def random_rows(n_cols, seed):
    """m rows at the full stride, three quarters of the bits set, the pad behind the last column included."""
    rng = np.random.default_rng(seed)
    s = stride_of(n_cols)
    return np.ascontiguousarray(rng.integers(0, 256, (M, s), dtype=np.uint8) | rng.integers(0, 256, (M, s), dtype=np.uint8))


def plant(rows, ids, col, positions):
    """Column `col` cleared in every row, then set in all h rows of the chosen positions (ids: the sequence's row ids by position)."""
    rows[:, col >> 3] &= np.uint8(0xFF ^ (0x80 >> (col & 7)))
    if len(positions):
        rows[np.unique(ids[np.asarray(positions, np.int64)].astype(np.int64)), col >> 3] |= np.uint8(0x80 >> (col & 7))


PATTERNS = ("ones", "zero", "straddle", "seg_last", "twins", "start0")


def straddle_start(w):
    return SEG * (w // 2 // SEG + 1) - w // 2


def pattern_positions(name, n, w):
    """The positions of the main sequence (n of them, window w) that hold a pattern's column."""
    if name == "ones":
        return list(range(n))                                   # best_found = We: the overflow check at We = 2^P - 1 and 2^P
    if name == "zero":
        return []                                               # no hit
    if name == "straddle":
        start = straddle_start(w)
        return list(range(start, start + w))                    # the best window straddles a segment boundary in its middle
    if name == "seg_last":
        return list(range(SEG - 1, SEG - 1 + w))                # ... starts at the last start of a segment
    if name == "twins":
        return list(range(10, 10 + w)) + list(range(2 * w + 15, 3 * w + 15))      # two equal maxima, two islands of passing windows
    if name == "start0":
        return list(range(w))                                   # best at start 0: at t = 1 it passes in the warm-up window only
    raise KeyError(name)


def make_case(n_cols, h, w, seed):
    """rows, sequences and the planted columns {pattern: column} of one case.  The main sequence has 3 w + 150 positions; beside it a
    sequence of period w (the k-mer that enters a window is the one that leaves it), one of period w / 2 (a k-mer repeated inside a
    window), sequences shorter than k, of exactly k and empty, and sequences of w + 1, w and w - 1 positions (W = n - 1, n, > n)."""
    rng = np.random.default_rng(seed)
    n_main = 3 * w + 150
    main = rand_seq(rng, n_main + K - 1)
    reps = lambda unit, length: (unit * (length // len(unit) + 1))[:length]      # noqa: E731
    seqs = [main, rand_seq(rng, K - 1), reps(rand_seq(rng, w), 3 * w + K + 10), rand_seq(rng, K), "", reps(rand_seq(rng, max(w // 2, 1)), 2 * w + K + 20),
            rand_seq(rng, w + K), rand_seq(rng, w + K - 1)] + ([rand_seq(rng, w + K - 2)] if w > 1 else [])
    rows = random_rows(n_cols, seed + 1)
    ids = coracle.seq_rows(main, K, h, M)
    cols = [c for c in dict.fromkeys([0, n_cols - 1, 63, 64, 65, 127, 128]) if c < n_cols]
    planted = dict(zip(PATTERNS, cols))
    for name, c in planted.items():
        plant(rows, ids, c, pattern_positions(name, n_main, w))
    return rows, seqs, planted


def reference(rows, seqs, n_cols, h, w, t):
    return window_reference([presence_from_rows(rows, coracle.seq_rows(s, K, h, M), n_cols) for s in seqs], w, t)


def clean(h, w):
    """A planted pattern survives as planted: with fewer hashes, or with more planted positions, the positions of a sequence share
    too many of the 4096 rows (the expectation is taken from the bytes either way)."""
    return h >= 3 and w <= 16


def check_intent(rows, seqs, planted, n_cols, h, w):
    """The planted patterns are what they are meant to be, read off the reference (t = 1): run on the CPU."""
    pres = presence_from_rows(rows, coracle.seq_rows(seqs[0], K, h, M), n_cols)
    we, found = found_matrix(pres, w)
    assert we == w and found.shape[0] == 2 * w + 151
    for name, c in planted.items():
        f = found[:, c]
        if name == "ones":
            assert (f == w).all()
        elif name == "zero":
            assert (f == 0).all()
        elif clean(h, w):
            best = np.flatnonzero(f == w)
            if name == "straddle":
                assert best.tolist() == [straddle_start(w)] and (w == 1 or straddle_start(w) < SEG < straddle_start(w) + w)
            elif name == "seg_last":
                assert best.tolist() == [SEG - 1]
            elif name == "twins":
                assert best.tolist() == [10, 2 * w + 15]
            elif name == "start0":
                assert best.tolist() == [0]


class Raw(object):
    """One index straight on the C ABI holding `rows` (uint8[M, stride]: junk behind num_cols included)."""

    def __init__(self, rows, n, h, starts=SEG):
        from bigsi_amd import _lib
        self.L, self.lib = _lib.lib(), _lib
        self.n, self.h, self.rows = n, h, rows
        self.ix = C.c_void_p()
        _lib.check(self.L.bigsi_hip_open(M, n, n, h, 0, C.byref(self.ix)))
        inf = _lib.Info()
        _lib.check(self.L.bigsi_hip_get_info(self.ix, C.byref(inf)))
        assert int(inf.row_stride_bytes) == rows.shape[1], (int(inf.row_stride_bytes), rows.shape[1])
        ids = np.arange(M, dtype=np.uint64)
        _lib.check(self.L.bigsi_hip_set_rows(self.ix, ptr(ids), M, ptr(rows), rows.shape[1]))
        _lib.check(self.L.bigsi_hip_window_set_limits(self.ix, starts, 0))
        self.batches = []

    def want(self, seqs, w, t):
        return reference(self.rows, seqs, self.n, self.h, w, t)

    def search(self, seqs, w, t, capacity, handle=None, null=None, k=K):
        blob, off = pack(seqs)
        o = Outputs(len(seqs), capacity)
        a = {"used": ptr(o.used), "need": ptr(o.need), "off": ptr(o.off), "cols": ptr(o.cols), "recs": ptr(o.recs)}
        if null:
            a[null] = None
        rc = self.L.bigsi_hip_window_search(handle or self.ix, blob, ptr(off), len(seqs), k, w, t, a["used"], a["need"], a["off"], a["cols"], a["recs"], capacity)
        return rc, o

    def check(self, seqs, w, t, handle=None):
        want = self.want(seqs, w, t)
        rc, o = self.search(seqs, w, t, int(want[2][-1]), handle=handle)
        assert rc == 0, self.L.bigsi_hip_last_error()
        o.assert_equal(want)
        return want

    def batch(self, seqs):
        blob, off = pack(seqs)
        b = C.c_void_p()
        self.lib.check(self.L.bigsi_hip_batch_create(self.ix, blob, ptr(off), len(seqs), K, C.byref(b)))
        self.batches.append(b)
        return b

    def batch_search(self, b, n_seqs, w, t, capacity, null=None):
        o = Outputs(n_seqs, capacity)
        a = {"used": ptr(o.used), "need": ptr(o.need), "off": ptr(o.off), "cols": ptr(o.cols), "recs": ptr(o.recs)}
        if null:
            a[null] = None
        return self.L.bigsi_hip_batch_window_search(b, w, t, a["used"], a["need"], a["off"], a["cols"], a["recs"], capacity), o

    def close(self):
        for b in self.batches:
            self.lib.check(self.L.bigsi_hip_batch_destroy(b))
        self.lib.check(self.L.bigsi_hip_close(self.ix))


def run_case(n_cols, h, w, seed):
    rows, seqs, planted = make_case(n_cols, h, w, seed)
    check_intent(rows, seqs, planted, n_cols, h, w)
    ix = Raw(rows, n_cols, h)
    try:
        hits = 0
        for t in (1.0, 0.4):
            want = ix.check(seqs, w, t)
            hits += int(want[2][-1])
            used = want[0].tolist()
            assert used[0] == w and used[1] == 0 and used[3] == 1 and used[4] == 0 and used[6:] == [w, w] + ([w - 1] if w > 1 else [])
            lo = int(want[2][0])
            mine = {int(c): want[4][lo + j] for j, c in enumerate(want[3][lo:int(want[2][1])])}
            assert mine[planted["ones"]]["best_found"] == w and mine[planted["ones"]]["windows_passing"] == 2 * w + 151
            if "zero" in planted:
                assert planted["zero"] not in mine
            if clean(h, w) and t == 1.0 and "twins" in planted:
                r = mine[planted["twins"]]
                assert (r["best_start"], r["first_start"], r["last_start"], r["windows_passing"]) == (10, 10, 2 * w + 15, 2)
            if clean(h, w) and t == 1.0 and "start0" in planted:
                assert mine[planted["start0"]].tolist() == (w, 0, 0, 0, 1, 0)
        assert hits > 0
    finally:
        ix.close()


# --------------------------------------------------------------------------------------------- kernels against numpy
WINDOWS = [1, 2, 3, 15, 16, 255, 256]


@pytest.mark.parametrize("h,w", [(h, w) for h in (1, 3, 9) for w in WINDOWS] + [(3, 4095), (2, 4096)])
def test_patterns_windows_and_hashes(h, w):
    """Every planted pattern at every window edge (1, 2, 3; 15 / 16 and 255 / 256: a plane edge inside a bucket and at a bucket's edge;
    4095 / 4096: the 16-plane instance) with h = 1, 3 and the run-time route (9), on 200 columns: a tile of two words, lanes idle."""
    run_case(200, h, w, seed=1000 * h + w)


@pytest.mark.parametrize("n_cols,h,w", list(zip([1, 63, 64, 65, 127, 128, 129, 1000, 8191, 8192, 8193], itertools.cycle([3, 1, 9, 2, 4, 7, 5, 6]),
                                                [16, 255, 3, 256, 1, 15, 2, 17, 16, 64, 3])))
def test_widths(n_cols, h, w):
    """The word, lane-pair and wavefront-slice edges of the row, every compile-time h once."""
    run_case(n_cols, h, w, seed=7 * n_cols + h)


def test_segment_length_does_not_change_the_result():
    """A 3000-position sequence in segments of 64 starts and in the planner's own: identical outputs, both the reference's."""
    rng = np.random.default_rng(41)
    rows = random_rows(129, 42)
    seqs = [rand_seq(rng, 3000 + K - 1), rand_seq(rng, 500)]
    plant(rows, coracle.seq_rows(seqs[0], K, 3, M), 77, list(range(1000, 1100)) + list(range(2063, 2163)))
    outs = []
    for starts in (SEG, 0, 1, 2901):
        ix = Raw(rows, 129, 3, starts=starts)
        try:
            for t in (1.0, 0.5):
                want = ix.check(seqs, 100, t)
                rc, o = ix.search(seqs, 100, t, int(want[2][-1]))
                assert rc == 0
                outs.append((starts, t, o))
            assert 77 in want[3].tolist()
        finally:
            ix.close()
    for (_, t, o), (_, t2, o2) in zip(outs[:2], outs[2:]):
        assert t == t2 and all(np.array_equal(getattr(o, f), getattr(o2, f)) for f in ("used", "need", "off", "cols", "recs"))


def test_hit_lists_beyond_their_first_size():
    """More than 65536 hits in one call: the write pass of the compaction runs again on grown lists."""
    rng = np.random.default_rng(77)
    rows = random_rows(8193, 78)
    seqs = [rand_seq(rng, 200) for _ in range(10)]
    ix = Raw(rows, 8193, 1)
    try:
        want = ix.check(seqs, 3, 0.3)
        assert int(want[2][-1]) > 65536
        ix.check(seqs[:2], 3, 1.0)
    finally:
        ix.close()


def canonical(kmer):
    rc = kmer[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return min(kmer, rc)


def test_one_window_equals_the_shipped_search():
    """W >= n: one window, so colours and best_found are bigsi_hip_search_batch's colours and counts at the same threshold --
    provided no k-mer occurs twice (a search counts unique k-mers, a window positions), which is asserted here on the CPU."""
    rng = np.random.default_rng(2024)
    seqs = [rand_seq(rng, 3000), rand_seq(rng, 500), rand_seq(rng, 100), rand_seq(rng, K)]
    # (no sequence without a k-mer here: a thresholded search gives such a query min_kmers = 0 and every sample, a window search nothing)
    for s in seqs:
        kmers = [canonical(s[i:i + K]) for i in range(max(len(s) - K + 1, 0))]
        assert len(set(kmers)) == len(kmers)
    rows = random_rows(1000, 5)
    for s in seqs:
        plant(rows, coracle.seq_rows(s, K, 3, M), 5, [])
    for s in seqs:          # column 5 holds every k-mer of all of them: a hit at t = 1
        ids = coracle.seq_rows(s, K, 3, M).astype(np.int64)
        rows[np.unique(ids), 0] |= np.uint8(0x80 >> 5)
    ix = Raw(rows, 1000, 3)
    try:
        blob, off = pack(seqs)
        for t in (1.0, 0.4):
            want = ix.check(seqs, 3000, t)
            total = int(want[2][-1])
            nk, nu, mk = (np.zeros(4, np.uint32) for _ in range(3))
            hoff, col, cnt = np.zeros(5, np.uint64), np.zeros(total + 8, np.uint32), np.zeros(total + 8, np.uint32)
            ix.lib.check(ix.L.bigsi_hip_search_batch(ix.ix, blob, ptr(off), 4, K, C.c_double(t), 0, ptr(nk), ptr(nu), ptr(mk), ptr(hoff), ptr(col), ptr(cnt), total + 8))
            assert np.array_equal(nk, nu) and np.array_equal(nu, want[0]) and np.array_equal(mk, want[1])
            assert np.array_equal(hoff, want[2]) and np.array_equal(col[:total], want[3]) and np.array_equal(cnt[:total], want[4]["best_found"])
            assert total >= 4 and want[3].tolist().count(5) == 4
            assert (want[4]["best_start"] == 0).all() and (want[4]["windows_passing"] == 1).all()
    finally:
        ix.close()


# --------------------------------------------------------------------------------------------- protocol
def test_protocol_of_both_calls():
    from bigsi_amd import _lib
    rng = np.random.default_rng(8)
    rows = random_rows(300, 9)
    ix = Raw(rows, 300, 3)
    view = C.c_void_p()
    ix.lib.check(ix.L.bigsi_hip_open_view(ix.ix, C.byref(view)))
    try:
        seqs = [rand_seq(rng, 400), rand_seq(rng, 10), rand_seq(rng, 150)]
        w, t = 50, 0.5
        want = ix.check(seqs, w, t)
        total = int(want[2][-1])
        assert total > 10
        # capacity: the offsets, windows and needs are filled, the lists untouched
        rc, o = ix.search(seqs, w, t, total - 1)
        assert rc == ERR_CAPACITY and b"needed" in ix.L.bigsi_hip_last_error() and o.lists_untouched()
        assert np.array_equal(o.off[:4], want[2]) and np.array_equal(o.used[:3], want[0]) and np.array_equal(o.need[:3], want[1])
        rc, o = ix.search(seqs, w, t, 0, null="cols")
        assert rc == ERR_CAPACITY and np.array_equal(o.off[:4], want[2])
        # invalid arguments: nothing is written
        for bad_w, bad_t in ((0, t), (65536, t), (w, 0.0), (w, -1.0), (w, 1.5), (w, float("nan"))):
            rc, o = ix.search(seqs, bad_w, bad_t, total)
            assert rc == ERR_INVALID and (o.off == SENTINEL).all() and (o.used == SENTINEL).all() and (o.need == SENTINEL).all() and o.lists_untouched()
        for null in ("used", "need", "off", "cols", "recs"):
            assert ix.search(seqs, w, t, total, null=null)[0] == ERR_INVALID, null
        assert ix.search(seqs, w, t, total, k=0)[0] == ERR_INVALID
        blob, off = pack(seqs)
        o = Outputs(3, total)
        assert ix.L.bigsi_hip_window_search(None, blob, ptr(off), 3, K, w, t, ptr(o.used), ptr(o.need), ptr(o.off), ptr(o.cols), ptr(o.recs), total) == ERR_INVALID
        assert ix.L.bigsi_hip_window_search(ix.ix, blob, ptr(off), 0, K, w, t, ptr(o.used), ptr(o.need), ptr(o.off), ptr(o.cols), ptr(o.recs), total) == ERR_INVALID
        assert ix.L.bigsi_hip_window_search(ix.ix, blob, None, 3, K, w, t, ptr(o.used), ptr(o.need), ptr(o.off), ptr(o.cols), ptr(o.recs), total) == ERR_INVALID
        # the handle is fine afterwards; the same workspace takes a smaller and a larger load; a view handle gives the owner's numbers
        ix.check(seqs, w, t)
        ix.check([rand_seq(rng, 60)], w, 1.0)
        ix.check(seqs + [rand_seq(rng, 900)], 255, 0.45)
        ix.lib.check(ix.L.bigsi_hip_window_set_limits(view, SEG, 0))
        ix.check(seqs, w, t, handle=view)
        # only sequences without k-mers
        rc, o = ix.search(["ACGT", ""], w, t, 4)
        assert rc == 0 and o.off[:3].tolist() == [0, 0, 0] and o.used[:2].tolist() == [0, 0] and o.need[:2].tolist() == [0, 0] and o.lists_untouched()
        # the batch call: not before a run; after an exact and after a thresholded run; the batch's own hit lists stay
        b = ix.batch(seqs)
        rc, o = ix.batch_search(b, 3, w, t, total)
        assert rc == ERR_STATE and (o.off == SENTINEL).all() and o.lists_untouched()
        for run_t in (1.0, 0.4):
            ix.lib.check(ix.L.bigsi_hip_batch_run(b, C.c_double(run_t), 0))
            hoff, col, cnt = np.zeros(4, np.uint64), np.zeros(900, np.uint32), np.zeros(900, np.uint32)
            ix.lib.check(ix.L.bigsi_hip_batch_fetch_hits(b, ptr(hoff), ptr(col), ptr(cnt), 900))
            rc, o = ix.batch_search(b, 3, w, t, total)
            assert rc == 0, ix.L.bigsi_hip_last_error()
            o.assert_equal(want)
            hoff2, col2, cnt2 = np.zeros(4, np.uint64), np.zeros(900, np.uint32), np.zeros(900, np.uint32)
            ix.lib.check(ix.L.bigsi_hip_batch_fetch_hits(b, ptr(hoff2), ptr(col2), ptr(cnt2), 900))
            assert np.array_equal(hoff, hoff2) and np.array_equal(col, col2) and np.array_equal(cnt, cnt2)
        rc, o = ix.batch_search(b, 3, w, t, total - 1)
        assert rc == ERR_CAPACITY and np.array_equal(o.off[:4], want[2]) and o.lists_untouched()
        assert ix.batch_search(b, 3, 0, t, total)[0] == ERR_INVALID and ix.batch_search(b, 3, w, 2.0, total)[0] == ERR_INVALID
        assert ix.batch_search(b, 3, w, t, total, null="off")[0] == ERR_INVALID
        assert ix.L.bigsi_hip_batch_window_search(None, w, C.c_double(t), ptr(o.used), ptr(o.need), ptr(o.off), ptr(o.cols), ptr(o.recs), total) == ERR_INVALID
        # a reload: not before the next run, then the new sequences' answer
        other = [rand_seq(rng, 200), rand_seq(rng, 333)]
        blob2, off2 = pack(other)
        ix.lib.check(ix.L.bigsi_hip_batch_reload(b, blob2, ptr(off2), 2, K))
        assert ix.batch_search(b, 2, w, t, 900)[0] == ERR_STATE
        ix.lib.check(ix.L.bigsi_hip_batch_run(b, C.c_double(1.0), 0))
        want2 = ix.want(other, w, t)
        rc, o = ix.batch_search(b, 2, w, t, int(want2[2][-1]))
        assert rc == 0
        o.assert_equal(want2)
        # num_hashes changed since the run
        ix.lib.check(ix.L.bigsi_hip_set_num_hashes(ix.ix, 2))
        rc, o = ix.batch_search(b, 2, w, t, 900)
        assert rc == ERR_STATE and b"num_hashes" in ix.L.bigsi_hip_last_error()
        ix.lib.check(ix.L.bigsi_hip_set_num_hashes(ix.ix, 3))
        assert ix.batch_search(b, 2, w, t, 900)[0] == 0
        # a batch of explicit k-mers
        s = rand_seq(rng, K + 1)
        kmers = [canonical(s[i:i + K]) for i in range(2)]
        eb = C.c_void_p()
        eoff, soff, pu, poff = np.asarray([0, K, 2 * K], np.uint64), np.asarray([0, 2], np.uint64), np.asarray([0, 1], np.uint32), np.asarray([0, 2], np.uint64)
        ix.lib.check(ix.L.bigsi_hip_batch_create_elements(ix.ix, "".join(kmers).encode(), ptr(eoff), ptr(soff), ptr(pu), ptr(poff), 1, C.byref(eb)))
        ix.batches.append(eb)
        ix.lib.check(ix.L.bigsi_hip_batch_run(eb, C.c_double(1.0), 0))
        rc, o = ix.batch_search(eb, 1, w, t, 900)
        assert rc == ERR_STATE and b"explicit" in ix.L.bigsi_hip_last_error() and (o.off == SENTINEL).all()
        # the forced cap on the per-segment maxima: refused with the numbers, and fine again without it
        assert ix.L.bigsi_hip_window_set_limits(None, 0, 0) == ERR_INVALID and ix.L.bigsi_hip_window_set_limits(ix.ix, 1 << 31, 0) == ERR_INVALID
        ix.lib.check(ix.L.bigsi_hip_window_set_limits(ix.ix, SEG, 1024))
        rc, o = ix.search(seqs, w, t, total)
        assert rc == ERR_INVALID and b"cap 1024" in ix.L.bigsi_hip_last_error() and o.lists_untouched()
        ix.lib.check(ix.L.bigsi_hip_window_set_limits(ix.ix, SEG, 0))
        ix.check(seqs, w, t)
    finally:
        ix.lib.check(ix.L.bigsi_hip_close(view))
        ix.close()


# --------------------------------------------------------------------------------------------- BIGSI level
KB, MB, HB = 21, 100003, 3


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """Four samples of 2 kbp; the query is 6.4 kbp of noise around 400 bp of sample s2.  The expectation comes from the samples' own
    Bloom filters and the oracle's row ids, so a Bloom false positive counts on both sides."""
    from bigsi_amd import BIGSI
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(99)
    samples = {"s%d" % i: rand_seq(rng, 2000) for i in range(4)}
    query = rand_seq(rng, 3000) + samples["s2"][500:900] + rand_seq(rng, 3000)
    d = tmp_path_factory.mktemp("window")
    c = {"storage-engine": "hip-hbm", "k": KB, "m": MB, "h": HB, "storage-config": {"name": "window%d" % next(_counter), "filename": str(d / "index.hbm")}}
    b = BIGSI.build_from_sequences(c, {n: [s] for n, s in samples.items()})
    filters = np.stack([np.unpackbits(np.frombuffer(BIGSI.bloom(c, list(seq_to_kmers(s, KB))).tobytes(), dtype=np.uint8))[:MB].astype(bool) for s in samples.values()])
    ids = coracle.seq_rows(query, KB, HB, MB).astype(np.int64)
    pres = filters[:, ids].all(axis=2).T          # [positions, samples]
    yield {"b": b, "cfg": c, "dir": d, "query": query, "pres": pres}
    b.delete()


def test_end_to_end_local_match(built):
    b, query, pres = built["b"], built["query"], built["pres"]
    w, t = 300, 0.9
    used, need, off, cols, recs = window_reference([pres], w, t)
    r = b.search_windows(query, w, t)
    assert list(r) == ["num_kmers", "window", "min_found", "results"]
    assert (r["num_kmers"], r["window"], r["min_found"]) == (len(query) - KB + 1, 300, 270)
    assert cols.tolist() == [2] and [x["sample_name"] for x in r["results"]] == ["s2"]
    x, want = r["results"][0], recs[0]
    assert (x["colour"], x["best_found"], x["best_start"], x["windows_passing"]) == (2, int(want["best_found"]), int(want["best_start"]), int(want["windows_passing"]))
    assert (x["match_start"], x["match_end"]) == (int(want["first_start"]), int(want["last_start"]) + w + KB - 1)
    # the embedded stretch is bases [3000, 3400): 380 positions; a window of 300 passes from 30 before it to 30 behind its last full start
    assert x["best_found"] == 300 and abs(x["match_start"] - 2970) <= 3 and abs(x["match_end"] - 3430) <= 3 and x["percent_found"] == 100.0
    # the plain search of the same query at the same threshold does not find the sample
    assert b.search(query, t) == [] or all(h["sample_name"] != "s2" for h in b.search(query, t))
    # many, and a deleted sample
    many = b.search_windows_many([query, "ACGT", query[2900:3500]], w, t)
    assert many[0] == r and many[1] == {"num_kmers": 0, "window": 0, "min_found": 0, "results": []}
    assert [y["sample_name"] for y in many[2]["results"]] == ["s2"] and many[2]["results"][0]["match_start"] == x["match_start"] - 2900
    assert b.search_windows_many([], w) == []
    with pytest.raises(ValueError):
        b.search_windows(query, 0)
    with pytest.raises(ValueError):
        b.search_windows("ACGTé" * 9, 5)


def test_cli_window_search(built, capsys):
    """`python -m bigsi_amd window_search` in a process of its own on the index's snapshot; the CSV form through the same main()."""
    from bigsi_amd.__main__ import main
    b, d, query = built["b"], built["dir"], built["query"]
    b.storage.sync()
    cf = d / "config.yaml"
    cf.write_text(yaml.safe_dump(built["cfg"]))
    want = dict({"query": query}, **b.search_windows(query, 300, 0.9))
    r = subprocess.run([sys.executable, "-m", "bigsi_amd", "window_search", query, "--window", "300", "-t", "0.9", "--config", str(cf)], cwd=str(d),
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == json.dumps([want]) + "\n" and json.loads(r.stdout)[0]["results"][0]["sample_name"] == "s2"
    fa = d / "q.fa"
    fa.write_text(">a\n%s\n>b\nACGT\n" % query)
    capsys.readouterr()
    assert main(["window_search", "--fasta", str(fa), "--window", "300", "-t", "0.9", "--format", "csv", "--config", str(cf)]) == 0
    rows = list(csv.reader(io.StringIO(capsys.readouterr().out)))
    x = want["results"][0]
    assert rows == [["record", "sample_name", "colour", "best_found", "percent_found", "best_start", "match_start", "match_end", "windows_passing"],
                    ["0", "s2", "2", str(x["best_found"]), "100.0", str(x["best_start"]), str(x["match_start"]), str(x["match_end"]), str(x["windows_passing"])]]


def test_deleted_sample_is_dropped(built):
    b, query = built["b"], built["query"]
    assert [x["sample_name"] for x in b.search_windows(query, 300, 0.9)["results"]] == ["s2"]
    b.delete_sample("s2")
    assert b.search_windows(query, 300, 0.9)["results"] == []
