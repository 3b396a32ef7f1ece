"""Support shared by tests/test_tally_host.py and tests/test_gpu_tally.py (a plain module: nothing here is collected): the numpy
reference of the query-set tally (include/bigsi_hip_tally.h) -- oracle.coracle's hashing plus the row bytes, the method of
count_staircase's reference() --, the test indexes with hits planted at the edge columns, and a plain Python restatement of the host
planners plan_tally / plan_tally_chunks (csrc/bigsi_launch.hpp) that the host test pins against the compiled header.

The planted index.  M rows, H hashes, K = 31; a background of 2 % random bits; per query i and edge column e_j (column 0, 63, 64, the
first and the last column of the last result word = n - 1) a role (i + j) % 3: 0 -- every row of every k-mer of the query is set in the
column (a hit at any threshold), 1 -- the rows of the first half of its k-mers (a partial count: a hit below threshold 1 only), 2 --
nothing.  From three queries on, query 1 hits nothing (its rows are cleared in every column, after the planting) and query 2 is shorter
than k.  Counts are whatever the finished matrix gives (rows collide): the reference is computed from the matrix, never from the plan,
and the host test asserts the conditions the GPU cases rely on."""
import math

import numpy as np

from oracle import coracle
from raw_index import rand_seq

K, M, H = 31, 40009, 3

# --------------------------------------------------------------------------------------------- the planners, restated
BLOCK, TILE, LOADS, TOTALS_TILE = 256, 128, 8, 4
CHUNK_SEQS, CHUNK_POSITIONS, COUNTER_BYTES = 4096, 1 << 20, 2 << 30


def plan_tally(n_seqs, wv):
    word_groups, tiles = -(-wv // (BLOCK // 64)), -(-n_seqs // TILE)
    grid = word_groups * tiles
    return dict(block=BLOCK, tile=TILE, word_groups=word_groups, tiles=tiles, grid=grid, totals_grid=-(-n_seqs // TOTALS_TILE),
                too_large=grid if grid > 0x7FFFFFFF else 0)


def plan_tally_chunks(lengths, k, wv_pad, count_bytes):
    """cuts: chunk i is the sequences [cuts[i], cuts[i + 1])"""
    n, per_seq = len(lengths), wv_pad * 64 * count_bytes
    by_bytes = max(COUNTER_BYTES // per_seq, 1) if per_seq else CHUNK_SEQS
    cuts = [0]
    while cuts[-1] < n:
        s0 = s = cuts[-1]
        most, pos = min(CHUNK_SEQS, by_bytes, n - s0), 0
        while s < s0 + most:
            p = max(lengths[s] - k + 1, 0)
            if s > s0 and pos + p > CHUNK_POSITIONS:
                break
            pos += p
            s += 1
        cuts.append(s)
    return cuts


# --------------------------------------------------------------------------------------------- the reference
def min_kmers(u, thr):
    """the device's ceil((double)u * t), clamped at 0"""
    return max(int(math.ceil(u * thr)), 0)


def counts_of(dense, n_cols, h, seq, k=K):
    """(u, int64[n_cols]): per column the number of the sequence's distinct k-mers whose h rows all have the column set"""
    first, _ = coracle.unique_kmers(seq, k)
    if len(first) == 0:
        return 0, np.zeros(n_cols, np.int64)
    rows = coracle.seq_rows(seq, k, h, dense.shape[0])[first].astype(np.int64)
    a = dense[rows[:, 0]]
    for j in range(1, h):
        a = a & dense[rows[:, j]]
    return len(first), np.unpackbits(a, axis=1)[:, :n_cols].sum(axis=0, dtype=np.int64)


def tally_of(us, counts, thr):
    """(queries_hit uint64[n_cols], kmers_found uint64[n_cols], totals uint64[4]) of queries with `us` unique k-mers and per-column
    `counts` at threshold thr -- the definition, line by line"""
    us, counts = np.asarray(us, np.int64), np.asarray(counts, np.int64)
    mk = np.array([min_kmers(int(u), thr) for u in us], np.int64)
    hit = (counts >= mk[:, None]) & (us > 0)[:, None]
    totals = np.array([(us > 0).sum(), us.sum(), (us == 0).sum(), hit.any(axis=1).sum()], np.uint64)
    return hit.sum(axis=0).astype(np.uint64), np.where(hit, counts, 0).sum(axis=0).astype(np.uint64), totals


def add(a, b):
    return tuple(x + y for x, y in zip(a, b))


# --------------------------------------------------------------------------------------------- the planted index
def edge_columns(n_cols):
    wv = -(-n_cols // 64)
    return sorted({c for c in (0, 63, 64, n_cols - 1, 64 * (wv - 1)) if 0 <= c < n_cols})


class Planted(object):
    """seqs, dense (uint8[M, ceil(n_cols / 8)], pad bits zero), n_cols, us (int64[n]) and counts (int64[n, n_cols], read-only)"""

    def __init__(self, n_cols, n_seqs, seed, lengths=None):
        rng = np.random.default_rng(seed)
        self.n_cols, self.edges = n_cols, edge_columns(n_cols)
        lengths = list(lengths) if lengths is not None else [K + int(rng.integers(8, 60)) for _ in range(n_seqs)]
        self.zero_hit, self.short = (1, 2) if n_seqs >= 3 else (None, None)
        if self.short is not None:
            lengths[self.short] = 20
        self.seqs = [rand_seq(rng, n) for n in lengths]
        bits = (rng.random((M, n_cols), dtype=np.float32) < 0.02).astype(np.uint8)
        rows_of = []
        for s in self.seqs:
            first, _ = coracle.unique_kmers(s, K)
            rows_of.append(coracle.seq_rows(s, K, H, M)[first].astype(np.int64))
        for i, rows in enumerate(rows_of):
            if i in (self.zero_hit, self.short):
                continue
            for j, e in enumerate(self.edges):
                role = (i + j) % 3
                if role == 0:
                    bits[rows.ravel(), e] = 1
                elif role == 1:
                    bits[rows[:(len(rows) + 1) // 2].ravel(), e] = 1
        if self.zero_hit is not None:
            bits[rows_of[self.zero_hit].ravel(), :] = 0
        self.dense = np.packbits(bits, axis=1)
        pairs = [counts_of(self.dense, n_cols, H, s) for s in self.seqs]
        self.us = np.array([u for u, _ in pairs], np.int64)
        self.counts = np.stack([c for _, c in pairs])
        self.counts.setflags(write=False)

    def edge_threshold(self):
        """A threshold below 1 whose min_kmers, for some query, is EXACTLY the count an edge column holds (0 < count < u): `>=` hits
        it, `>` would not.  Returns (thr, query, column)."""
        for i, u in enumerate(self.us):
            for e in self.edges:
                c = int(self.counts[i, e])
                if 0 < c < u:
                    thr = (c - 0.5) / int(u)
                    if min_kmers(int(u), thr) == c:
                        return thr, i, e
        raise AssertionError("no edge column holds a partial count")

    def tally(self, thr, sel=None):
        sel = slice(None) if sel is None else sel
        return tally_of(self.us[sel], self.counts[sel], thr)

    def junk_rows(self, stride, seed=7):
        """The rows at the full stride: every bit behind the last column -- the rest of the last byte and the padding -- random."""
        rng = np.random.default_rng(seed)
        full = rng.integers(0, 256, size=(M, stride), dtype=np.uint8)
        rb = self.dense.shape[1]
        full[:, :rb - 1] = self.dense[:, :rb - 1]
        pad = np.uint8(0xFF >> (self.n_cols & 7)) if self.n_cols & 7 else np.uint8(0)
        full[:, rb - 1] = self.dense[:, rb - 1] | (full[:, rb - 1] & pad)
        return np.ascontiguousarray(full)


_planted = {}


def planted(n_cols, n_seqs, seed=0, lengths=None):
    """built once per process and shared; nobody changes them"""
    key = (n_cols, n_seqs, seed, None if lengths is None else tuple(lengths))
    if key not in _planted:
        _planted[key] = Planted(n_cols, n_seqs, seed, lengths)
    return _planted[key]


def stream_lengths():
    """The input of the add_stream GPU case: cut into 3 chunks (tests/test_tally_host.py pins the cuts), the middle one a single
    sequence of more than 2^20 k-mer positions; query 1 hits nothing and query 2 is shorter than k, as in every planted case."""
    return [K + 40, K + 40, 20, K + 40, K + 40, (1 << 20) + 200 + K - 1] + [K + 25] * 6


def check_conditions(p, thr):
    """What a case must hold so that a GPU comparison at threshold `thr` cannot pass vacuously (from three queries on)."""
    qh, kf, totals = p.tally(thr)
    n = len(p.seqs)
    mk = np.array([min_kmers(int(u), thr) for u in p.us], np.int64)
    hit = (p.counts >= mk[:, None]) & (p.us > 0)[:, None]
    assert ((qh > 0) & (qh < n)).any(), "no sample is hit by some but not all queries"
    assert int(totals[2]) >= 1 and p.us[p.short] == 0, "no query shorter than k"
    assert not hit[p.zero_hit].any() and p.us[p.zero_hit] > 0, "no query that hits nothing"
    assert all(qh[e] > 0 for e in p.edges), "an edge column without a hit"
    if thr < 1.0:
        # some sample's hits found different numbers of k-mers: its kmers_found is not its queries_hit times any one number
        lo, hi = np.where(hit, p.counts, np.iinfo(np.int64).max).min(axis=0), np.where(hit, p.counts, -1).max(axis=0)
        assert ((qh > 0) & (lo != hi)).any(), "kmers_found is queries_hit times a constant"
