"""Read classification on the device (include/bigsi_hip_classify.h), straight on the C ABI: k_classify_groups in its three instances
(<uint16_t, EXACT>, <uint16_t>, <uint32_t>) against numpy -- oracle.coracle's hashing plus the row bytes (tests/classify_ref.py over
tally_ref's planted indexes), never a library call -- on indexes written by bigsi_hip_set_rows with junk bits behind num_cols.  Width
edges and query counts under two group layouts at threshold 1, at a threshold whose min_kmers sits exactly on a count an edge column
holds and at 0, dense and hits-only counters, both counter widths on the staircase cases, one group / 4096 groups / 4097 refused, one
query that hits every column, classify / reload / run / classify and destroy-behind-classify without a host wait, classify_stream over
three chunks (one of them a single sequence of 2^20 + 200 positions) and over a chunk of nothing but short sequences, every refusal
with preset outputs, a view handle, and BIGSI.classify / `python -m bigsi_amd classify` end to end with a deleted sample and --others.
tests/test_classify_host.py asserts, on the CPU, that none of the references is vacuous."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import yaml

import classify_ref as R
import tally_ref as T
from count_staircase import K as SK, build_case
from raw_index import Raw, ptr, rand_seq
from test_classify_host import QUERY_COUNTS, WIDTHS, same, width_case

pytestmark = pytest.mark.gpu
_counter = itertools.count()
SKIP_COMPACT, SPARSE_COUNTS = 2, 8
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6


@pytest.fixture(scope="module", autouse=True)
def hip():
    from bigsi_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible"


class Dev(object):
    """An index on the device and the calls under test, as the C ABI has them."""

    def __init__(self, m, n_cols, h, row_ids, rows):
        self.raw = Raw(m, n_cols, h=h)
        self.L, self.lib, self.ix, self.n_cols = self.raw.L, self.raw.lib, self.raw.ix, n_cols
        ids = np.ascontiguousarray(row_ids, dtype=np.uint64)
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        self.lib.check(self.L.bigsi_hip_set_rows(self.ix, ptr(ids), ids.size, ptr(rows), rows.shape[1]))

    @classmethod
    def planted(cls, p):
        probe = Raw(T.M, p.n_cols, h=T.H)
        stride = probe.stride
        probe.close()
        return cls(T.M, p.n_cols, T.H, np.arange(T.M), p.junk_rows(stride))

    def batch(self, seqs, k=T.K, handle=None):
        blob, off = self.lib.pack_seqs(seqs)
        b = C.c_void_p()
        self.lib.check(self.L.bigsi_hip_batch_create(handle or self.ix, blob, ptr(off), len(seqs), k, C.byref(b)))
        return b

    def reload(self, b, seqs, k=T.K):
        blob, off = self.lib.pack_seqs(seqs)
        self.lib.check(self.L.bigsi_hip_batch_reload(b, blob, ptr(off), len(seqs), k))

    def run(self, b, thr, flags=SKIP_COMPACT):
        self.lib.check(self.L.bigsi_hip_batch_run(b, float(thr), flags))

    def info(self, b):
        inf = self.lib.BatchInfo()
        self.lib.check(self.L.bigsi_hip_batch_get_info(b, C.byref(inf)))
        return inf

    def free(self, b):
        self.lib.check(self.L.bigsi_hip_batch_destroy(b))

    def classify_rc(self, b, n_seqs, g, n_groups, capacity=None, n_entries=None):
        """(rc, records) over a buffer preset to a pattern, with a guard record behind n_seqs"""
        rec = np.zeros(n_seqs + 1, R.DTYPE)
        rec.view(np.uint8)[:] = 0xAB
        rc = self.L.bigsi_hip_classify_batch(b, ptr(g), g.size if n_entries is None else n_entries, n_groups, ptr(rec), n_seqs if capacity is None else capacity)
        assert rec[-1].tobytes() == b"\xab" * 48
        return rc, rec[:-1]

    def classify(self, b, n_seqs, g, n_groups):
        rc, rec = self.classify_rc(b, n_seqs, g, n_groups)
        assert rc == 0, self.raw.err()
        return rec

    def stream_rc(self, seqs, thr, g, n_groups, k=T.K, handle=None, n_entries=None):
        blob, off = self.lib.pack_seqs(seqs)
        rec = np.zeros(len(seqs) + 1, R.DTYPE)
        rec.view(np.uint8)[:] = 0xAB
        rc = self.L.bigsi_hip_classify_stream(handle or self.ix, blob, ptr(off), len(seqs), k, float(thr), ptr(g), g.size if n_entries is None else n_entries, n_groups, ptr(rec))
        assert rec[-1].tobytes() == b"\xab" * 48
        return rc, rec[:-1]

    def stream(self, seqs, thr, g, n_groups, k=T.K, handle=None):
        rc, rec = self.stream_rc(seqs, thr, g, n_groups, k, handle)
        assert rc == 0, self.raw.err()
        return rec

    def close(self):
        self.raw.close()


def untouched(rec):
    return rec.tobytes() == b"\xab" * (48 * len(rec))


def check_planted(p, what):
    """one batch of all queries at the three thresholds -- 1.0 is the EXACT instance, the others read counters, dense and hits-only --
    under both layouts, each run classified twice over"""
    d = Dev.planted(p)
    b = d.batch(p.seqs)
    n = len(p.seqs)
    try:
        for thr in R.thresholds(p):
            for flags in ((SKIP_COMPACT,) if thr == 1.0 else (SKIP_COMPACT, SKIP_COMPACT | SPARSE_COUNTS)):
                d.run(b, thr, flags)
                assert d.info(b).exact == (1 if thr == 1.0 else 0)
                for name in R.LAYOUTS:
                    g, n_groups = R.layout(name, p.n_cols)
                    same(d.classify(b, n, g, n_groups), R.planted_records(p, thr, name), (what, thr, flags, name))
    finally:
        d.free(b)
        d.close()


@pytest.mark.parametrize("n_cols", WIDTHS)
def test_width_edges(n_cols):
    p = width_case(n_cols)
    if n_cols not in R.CONDITION_WIDTHS:
        assert len(p.seqs) == 5
    check_planted(p, ("width", n_cols))


@pytest.mark.parametrize("n_seqs", QUERY_COUNTS)
def test_query_counts(n_seqs):
    check_planted(T.planted(200, n_seqs, seed=n_seqs), ("queries", n_seqs))


# --------------------------------------------------------------------------------------------- counter widths: the staircase cases
_stair = {}


def stair_reference(name):
    """(us, counts) of every query of a staircase case: computed once, shared, never changed"""
    if name not in _stair:
        _, sc, queries = build_case(name)
        pairs = [sc.reference(q) for q in queries]
        _stair[name] = (np.array([u for u, _ in pairs], np.int64), np.stack([c for _, c in pairs]))
        _stair[name][1].setflags(write=False)
    return _stair[name]


@pytest.mark.parametrize("name, count_bytes", [("Uplain10", 2), ("S32", 4), ("S10b", 2)])
def test_counter_widths(name, count_bytes):
    c, sc, queries = build_case(name)
    us, counts = stair_reference(name)
    probe = Raw(c["m"], c["n_cols"], h=c["h"])
    stride = probe.stride
    probe.close()
    rows = np.random.default_rng(3).integers(0, 256, size=(sc.row_ids.size, stride), dtype=np.uint8)          # junk behind num_cols (whole bytes)
    assert c["n_cols"] % 8 == 0
    rows[:, :sc.packed.shape[1]] = sc.packed
    d = Dev(c["m"], c["n_cols"], c["h"], sc.row_ids, rows)
    b = d.batch(queries, SK)
    g, n_groups = R.layout("edges", c["n_cols"])
    g2, n_groups2 = R.layout("spread", c["n_cols"])
    # a layout of the case's own: the columns that hold the same count of the main query are one group, so that every group's found is
    # another number (the staircase's steps), read from the right counter or not at all
    steps, g3 = np.unique(counts[0], return_inverse=True)
    g3, n_groups3 = g3.astype(np.uint32), len(steps)
    assert n_groups3 >= 20
    try:
        for thr in sc.thresholds + [0.0]:
            wants = [(what, gg, n, R.records_of(us, counts, thr, gg, n)) for what, gg, n in (("edges", g, n_groups), ("spread", g2, n_groups2), ("steps", g3, n_groups3))]
            for flags in (SKIP_COMPACT, SKIP_COMPACT | SPARSE_COUNTS):
                d.run(b, thr, flags)
                inf = d.info(b)
                assert inf.exact == 0 and inf.count_bytes == count_bytes == c["route"]["count_bytes"], (name, thr)
                for what, gg, n, want in wants:
                    same(d.classify(b, len(queries), gg, n), want, (name, thr, flags, what))
            # the main query under "steps": the two highest steps, in order, each at its lowest column
            assert want["groups_hit"][0] >= 2 and (want["best_found"][0], want["second_found"][0]) == (steps[-1], steps[-2]) and want["best_group"][0] == n_groups3 - 1
            assert want["best_colour"][0] == np.flatnonzero(counts[0] == steps[-1])[0] and (counts[0] == steps[-1]).sum() >= 2
    finally:
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- group-count edges, dense hits
def test_one_group_4096_groups_and_4097():
    """every column of a 4160-column index its own group bar the last 64; hits planted at groups 0, 4095 and in the ungrouped tail"""
    m, n_cols, h = 4001, 4160, 2
    rng = np.random.default_rng(9)
    seqs = [rand_seq(rng, T.K + 20), rand_seq(rng, T.K + 30), rand_seq(rng, 12), rand_seq(rng, T.K + 9)]
    from oracle import coracle
    bits = np.zeros((m, n_cols), np.uint8)
    plant = {0: (0, 4095, 4100), 1: (4095, 17, 4159), 3: ()}          # query -> columns that hold all of it
    for i, cols in plant.items():
        first, _ = coracle.unique_kmers(seqs[i], T.K)
        rows = coracle.seq_rows(seqs[i], T.K, h, m)[first].astype(np.int64)
        for c in cols:
            bits[rows.ravel(), c] = 1
        half = rows[:len(rows) // 2].ravel()
        bits[half, 2000 + i] = 1                                         # ... and one that holds half of it
    dense = np.packbits(bits, axis=1)
    pairs = [T.counts_of(dense, n_cols, h, s) for s in seqs]
    us, counts = np.array([u for u, _ in pairs], np.int64), np.stack([c for _, c in pairs])
    probe = Raw(m, n_cols, h=h)
    stride = probe.stride
    probe.close()
    rows = np.zeros((m, stride), np.uint8)
    rows[:, :dense.shape[1]] = dense
    d = Dev(m, n_cols, h, np.arange(m), rows)
    b = d.batch(seqs)
    many = np.arange(n_cols, dtype=np.uint32)
    many[4096:] = R.NONE
    one = np.zeros(n_cols, np.uint32)
    one[4096:] = R.NONE
    try:
        for thr in (1.0, 0.4, 0.0):
            d.run(b, thr, SKIP_COMPACT if thr == 1.0 else SKIP_COMPACT | SPARSE_COUNTS)
            want = R.records_of(us, counts, thr, many, 4096)
            same(d.classify(b, 4, many, 4096), want, ("4096 groups", thr))
            if thr == 1.0:
                assert tuple(want[0])[2:] == (2, 2, 0, us[0], 0, 1, 4095, us[0], 4095, 1) and tuple(want[1])[4:8] == (17, us[1], 17, 1) and want["groups_hit"][3] == 0
            if thr == 0.0:
                assert (want["groups_hit"][[0, 1, 3]] == 4096).all() and (want["samples_hit"][[0, 1, 3]] == 4096).all()
            want = R.records_of(us, counts, thr, one, 1)
            same(d.classify(b, 4, one, 1), want, ("one group", thr))
            assert (want["second_group"] == R.NONE).all() and want["groups_hit"].max() == 1
        rc, rec = d.classify_rc(b, 4, many, 4097)
        assert rc == ERR_INVALID and untouched(rec) and b"n_groups" in d.raw.err()
        rc, rec = d.classify_rc(b, 4, many, 0)
        assert rc == ERR_INVALID and untouched(rec)
    finally:
        d.free(b)
        d.close()


def test_one_query_hits_every_column():
    """threshold 0 on the 775-wide index: every grouped column issues its pair of table updates"""
    p = width_case(775)
    d = Dev.planted(p)
    b = d.batch(p.seqs[:1])
    try:
        for flags in (SKIP_COMPACT, SKIP_COMPACT | SPARSE_COUNTS):
            d.run(b, 0.0, flags)
            for name in R.LAYOUTS:
                g, n_groups = R.layout(name, 775)
                want = R.planted_records(p, 0.0, name)[:1]
                assert want["samples_hit"][0] == (g != R.NONE).sum() and want["groups_hit"][0] == n_groups
                same(d.classify(b, 1, g, n_groups), want, ("every column", flags, name))
    finally:
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- ordering
def test_classify_reload_run_classify_without_a_wait():
    p = T.planted(200, 65, seed=65)
    thr = p.edge_threshold()[0]
    first, rest = slice(0, 23), slice(23, None)
    g, n_groups = R.layout("edges", 200)
    d = Dev.planted(p)
    b = d.batch(p.seqs[first])
    try:
        for x in (1.0, thr):
            want = R.planted_records(p, x, "edges")
            d.run(b, x)
            same(d.classify(b, 23, g, n_groups), want[first], ("first", x))
            d.reload(b, p.seqs[rest])          # at once: no wait of the caller's in between
            d.run(b, x)
            same(d.classify(b, 42, g, n_groups), want[rest], ("reloaded", x))
            same(d.classify(b, 42, g, n_groups), want[rest], ("classified twice", x))
            d.reload(b, p.seqs[first])
        # a batch destroyed right behind its classification
        b3 = d.batch(p.seqs[rest])
        d.run(b3, thr)
        rec = d.classify(b3, 42, g, n_groups)
        d.free(b3)
        same(rec, R.planted_records(p, thr, "edges")[rest], "destroy behind classify")
    finally:
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- streaming
def test_stream_over_three_chunks():
    lengths = T.stream_lengths()
    p = T.planted(200, len(lengths), seed=12, lengths=lengths)
    assert T.plan_tally_chunks([len(s) for s in p.seqs], T.K, 4, 4) == [0, 5, 6, 12] and p.us[5] > (1 << 19)
    d = Dev.planted(p)
    try:
        for name in R.LAYOUTS:
            g, n_groups = R.layout(name, 200)
            for x in (1.0, p.edge_threshold()[0]):
                want = R.planted_records(p, x, name)
                assert (want["groups_hit"][:5] >= 1).any() and (want["groups_hit"][6:] >= 2).all()          # the outer chunks have verdicts ...
                assert x == 1.0 or (want["groups_hit"][5] >= 2 and want["best_found"][5] > 1 << 19)         # ... below threshold 1 the single-sequence chunk too
                same(d.stream(p.seqs, x, g, n_groups), want, ("stream", name, x))
        # one batch over another split gives the same records
        for part in (slice(0, 3), slice(3, 5), slice(6, None)):
            b = d.batch(p.seqs[part])
            d.run(b, 1.0)
            same(d.classify(b, len(p.seqs[part]), g, n_groups), R.planted_records(p, 1.0, name)[part], ("batches", part))
            d.free(b)
        # a call of nothing but short sequences never reaches the device; nor does such a chunk between two that do
        short = ["ACGT", "", "TTTTTTTT"]
        same(d.stream(short, 1.0, g, n_groups), R.empty_records(3), "short only")
        filler = ["ACGTACGTAC"] * 4096                              # a whole chunk (4096 sequences) without a k-mer position
        seqs = filler[:4091] + p.seqs[:5] + filler + p.seqs[6:]
        assert T.plan_tally_chunks([len(s) for s in seqs], T.K, 4, 0) == [0, 4096, 8192, 8198]
        got = d.stream(seqs, 1.0, g, n_groups)
        want = R.planted_records(p, 1.0, name)
        same(got[:4091], R.empty_records(4091), "the short head of a mixed chunk")
        same(got[4091:4096], want[:5], "behind the short head")
        same(got[4096:8192], R.empty_records(4096), "the chunk of short sequences")
        same(got[8192:], want[6:], "behind the chunk of short sequences")
    finally:
        d.close()


# --------------------------------------------------------------------------------------------- refusals and handles
def test_refusals():
    p = T.planted(65, 5)
    d = Dev.planted(p)
    L = d.L
    b = d.batch(p.seqs)
    g, n_groups = R.layout("edges", 65)
    blob, off = d.lib.pack_seqs(p.seqs)
    out = np.zeros(5, R.DTYPE)
    try:
        # NULL arguments
        for rc in (L.bigsi_hip_classify_batch(None, ptr(g), 65, n_groups, ptr(out), 5), L.bigsi_hip_classify_batch(b, None, 65, n_groups, ptr(out), 5),
                   L.bigsi_hip_classify_batch(b, ptr(g), 65, n_groups, None, 5), L.bigsi_hip_classify_stream(None, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, ptr(out)),
                   L.bigsi_hip_classify_stream(d.ix, blob, None, 5, T.K, 1.0, ptr(g), 65, n_groups, ptr(out)),
                   L.bigsi_hip_classify_stream(d.ix, blob, ptr(off), 5, T.K, 1.0, None, 65, n_groups, ptr(out)),
                   L.bigsi_hip_classify_stream(d.ix, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, None),
                   L.bigsi_hip_classify_stream(d.ix, None, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, ptr(out))):
            assert rc == ERR_INVALID and d.raw.err()
        # what a stream's arguments are refused for: outputs untouched
        down = off.copy()
        down[2] = down[1] - 1
        for n, k, x, o in ((0, T.K, 1.0, off), (5, 0, 1.0, off), (5, T.K, 1.5, off), (5, T.K, float("nan"), off), (5, T.K, 1.0, down)):
            rec = np.zeros(5, R.DTYPE)
            rec.view(np.uint8)[:] = 0xAB
            assert L.bigsi_hip_classify_stream(d.ix, blob, ptr(o), n, k, x, ptr(g), 65, n_groups, ptr(rec)) == ERR_INVALID and untouched(rec)
        # group_of: its length, n_groups, a value out of range (the column is named) -- batch and stream alike
        d.run(b, 1.0)
        bad = g.copy()
        bad[64] = n_groups
        for gg, n_entries, groups, word in ((g, 64, n_groups, b"64 entries"), (g, 66, n_groups, b"66 entries"), (g, None, 0, b"n_groups"), (g, None, 4097, b"n_groups"),
                                            (bad, None, n_groups, b"group_of[64]"), (g, None, 7, b"group_of[64]")):
            rc, rec = d.classify_rc(b, 5, gg, groups, n_entries=n_entries)
            assert rc == ERR_INVALID and untouched(rec) and word in d.raw.err(), (n_entries, groups, d.raw.err())
            rc, rec = d.stream_rc(p.seqs, 1.0, gg, groups, n_entries=n_entries)
            assert rc == ERR_INVALID and untouched(rec) and word in d.raw.err()
        # capacity: nothing written
        rc, rec = d.classify_rc(b, 5, g, n_groups, capacity=4)
        assert rc == ERR_CAPACITY and untouched(rec)
        # a batch that has not run; one whose run built hit lists
        fresh = d.batch(p.seqs)
        rc, rec = d.classify_rc(fresh, 5, g, n_groups)
        assert rc == ERR_STATE and untouched(rec) and b"not completed" in d.raw.err()
        d.free(fresh)
        for thr in (1.0, 0.5):
            d.run(b, thr, flags=0)
            rc, rec = d.classify_rc(b, 5, g, n_groups)
            assert rc == ERR_STATE and untouched(rec) and b"SKIP_COMPACT" in d.raw.err()
        # a result limit, caller-owned bit vectors, a result width
        d.run(b, 1.0)
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 5, None, 0))
        rc, rec = d.classify_rc(b, 5, g, n_groups)
        assert rc == ERR_STATE and untouched(rec) and b"limit" in d.raw.err()
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 0, None, 0))
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, C.c_void_p(d.info(b).d_bitmaps)))
        assert d.classify_rc(b, 5, g, n_groups)[0] == ERR_STATE
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, None))
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 64))
        assert d.classify_rc(b, 5, g, n_groups)[0] == ERR_STATE
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 0))
        # num_hashes changed since the run
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, 2))
        rc, rec = d.classify_rc(b, 5, g, n_groups)
        assert rc == ERR_STATE and untouched(rec) and b"num_hashes" in d.raw.err()
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, T.H))
        # ... and the batch is fine
        same(d.classify(b, 5, g, n_groups), R.planted_records(p, 1.0, "edges"), "after the refusals")
        # an index without columns
        empty = Raw(64, 0, cap=8, h=3)
        rc = L.bigsi_hip_classify_stream(empty.ix, blob, ptr(off), 5, T.K, 1.0, ptr(g), 0, n_groups, ptr(out))
        assert rc == ERR_STATE
        empty.close()
    finally:
        d.free(b)
        d.close()


def test_view_handle():
    p = T.planted(129, 5)
    thr = p.edge_threshold()[0]
    g, n_groups = R.layout("spread", 129)
    d = Dev.planted(p)
    view = C.c_void_p()
    d.lib.check(d.L.bigsi_hip_open_view(d.ix, C.byref(view)))
    b = d.batch(p.seqs, handle=view)
    try:
        for x in (1.0, thr):
            d.run(b, x)
            same(d.classify(b, 5, g, n_groups), R.planted_records(p, x, "spread"), ("view, batch", x))
            same(d.stream(p.seqs, x, g, n_groups, handle=view), R.planted_records(p, x, "spread"), ("view, stream", x))
    finally:
        d.free(b)
        d.lib.check(d.L.bigsi_hip_close(view))
        d.close()


# --------------------------------------------------------------------------------------------- end to end
KB, MB, HB = 11, 100003, 3


def test_bigsi_classify_and_command_line(tmp_path, capsys):
    """BIGSI.classify and `classify` on an index built from sequences, one sample deleted, with and without --others: the result, the
    TSV and the JSON are the host layer's (bigsi_amd/classify.py) for the numpy reference over the samples' own Bloom filters."""
    from bigsi_amd import BIGSI, classify
    from bigsi_amd.__main__ import main
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(41)
    probe, other = rand_seq(rng, 60), rand_seq(rng, 50)
    seqs = {"s0": rand_seq(rng, 200), "s1": rand_seq(rng, 100) + probe + rand_seq(rng, 60), "s2": rand_seq(rng, 300) + other, "s3": probe + rand_seq(rng, 150),
            "s4": rand_seq(rng, 90) + probe[:40] + other, "s5": rand_seq(rng, 250)}
    cfg = {"storage-engine": "hip-hbm", "k": KB, "m": MB, "h": HB, "storage-config": {"name": "classify%d" % next(_counter), "filename": str(tmp_path / "index.hbm")}}
    b = BIGSI.build_from_sequences(cfg, {n: [s] for n, s in seqs.items()})
    try:
        b.delete_sample("s3")
        queries = [probe, other, "ACGT", probe[5:45], rand_seq(rng, 70), seqs["s5"][20:90], other[:30] + probe[:30]]
        filters = np.stack([np.unpackbits(np.frombuffer(BIGSI.bloom(cfg, list(seq_to_kmers(s, KB))).tobytes(), dtype=np.uint8))[:MB] for s in seqs.values()], axis=1)
        dense = np.packbits(filters, axis=1)
        pairs = [T.counts_of(dense, 6, HB, q, KB) for q in queries]
        us, counts = [u for u, _ in pairs], np.stack([c for _, c in pairs])
        names = [b.colour_to_sample(c) for c in range(6)]
        assert names[3] != "s3"
        groups = [("s1", "P"), ("s4", "P"), ("s2", "O")]
        group_file = tmp_path / "groups.tsv"
        group_file.write_text("".join("%s\t%s\n" % sg for sg in groups))
        plans = {None: (np.array([R.NONE, 0, 1, R.NONE, 0, R.NONE], np.uint32), ["P", "O"]), "rest": (np.array([2, 0, 1, R.NONE, 0, 2], np.uint32), ["P", "O", "rest"])}
        b.storage.sync()
        cf, fa = tmp_path / "config.yaml", tmp_path / "q.fa"
        cf.write_text(yaml.safe_dump(cfg))
        fa.write_text("".join(">q%d\n%s\n" % (i, q) for i, q in enumerate(queries)))
        ids = ["q%d" % i for i in range(len(queries))]
        for others, (g, gn) in plans.items():
            for thr, margin in ((1.0, 1), (0.6, 1), (0.6, 25)):
                rec = R.records_of(us, counts, thr, g, len(gn))
                want = classify.result(rec, gn, names.__getitem__, margin)
                got = b.classify(queries, groups, threshold=thr, margin=margin, others=others)
                assert got == want, (others, thr, margin)
                assert b.classify(iter(queries), {"P": ["s1", "s4"], "O": ["s2"]}, threshold=thr, margin=margin, others=others) == want
                chunks = list(b.classify_arrays(queries, groups, threshold=thr, others=others, batch_kmers=4))          # many small slices
                assert len(chunks) > 1 and [s for c, _ in chunks for s in c] == queries
                same(np.concatenate([r for _, r in chunks]), rec, ("slices", others, thr))
                capsys.readouterr()
                argv = ["classify", str(fa), "--groups", str(group_file), "-t", str(thr), "--margin", str(margin), "--config", str(cf)] + (["--others", others] if others else [])
                assert main(argv) == 0
                assert capsys.readouterr().out == classify.to_tsv(want, ids) + "\n"
                assert main(argv + ["--format", "json"]) == 0
                assert capsys.readouterr().out == classify.to_json(want, ids) + "\n"
                assert main(argv + ["--summary-only"]) == 0
                assert capsys.readouterr().out == classify.to_tsv(want, ids, summary_only=True) + "\n"
            verdict = [r["verdict"] for r in b.classify(queries, groups, threshold=0.6, others=others)["records"]]
            assert verdict[2] == "skipped" and verdict[0] == "assigned"
            assert verdict[5] == ("assigned" if others else "unclassified")          # a stretch of s5, which no group lists
        res = b.classify(queries, groups, threshold=1.0)
        assert res["records"][0]["group"] == "P" and res["records"][0]["best_sample"] == "s1" and res["records"][1]["verdict"] == "ambiguous"          # `other` is whole in O and P
        assert b.classify([], groups) == {"groups": ["P", "O"], "records": [], "summary": {"reads": 0, "assigned": {"P": 0, "O": 0}, "ambiguous": 0, "unclassified": 0, "skipped": 0}}
        with pytest.raises(KeyError):
            b.classify(queries, [("s3", "P")])                      # a deleted sample cannot be listed
        assert json.loads(classify.to_json(res, ids))["summary"]["reads"] == len(queries)
    finally:
        b.delete()
