"""Group association on the device (include/bigsi_hip_associate.h), straight on the C ABI: k_group_masks and k_group_counts against
numpy -- oracle.coracle's hashing plus the row bytes (tests/associate_ref.py over tally_ref's planted indexes), never a library call --
on indexes written by bigsi_hip_set_rows with junk bits behind num_cols.  Width edges (65, 129 and 775 columns have an odd number of
result words: a pad word is there to be misread) under four group layouts at threshold 1, at a threshold whose min_kmers sits exactly
on a count an edge column holds and at 0, dense and hits-only counters; query counts around the kernel's queries per workgroup; group
counts around its group block, an empty group, no group at all, 0 and 65 refused; the hit-dense case; agreement with the classifier on
the same run; associate / reload / run / associate and destroy-behind-associate without a host wait; associate_stream over three chunks
(one of them a single sequence of 2^20 + 200 positions) and over a chunk of nothing but short sequences, twice, bit-identical; every
refusal with preset outputs; a view handle; and BIGSI.associate / `python -m bigsi_amd associate` end to end with a deleted sample and
--others.  No tolerance anywhere.  tests/test_associate_host.py asserts, on the CPU, that none of the references is vacuous."""
import ctypes as C
import itertools

import numpy as np
import pytest
import yaml

import associate_ref as R
import classify_ref as CR
import tally_ref as T
from raw_index import Raw, ptr, rand_seq
from test_associate_host import QUERY_COUNTS, WIDTHS, guards_hold, part, preset, same, untouched, width_case

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

    def associate_rc(self, b, n_seqs, g, n_groups, capacity=None, n_entries=None):
        """(rc, (counts, info)) over buffers preset to a pattern, with a guard entry behind n_seqs"""
        counts, info = preset(n_seqs, max(n_groups, 1))
        rc = self.L.bigsi_hip_associate_batch(b, ptr(g), g.size if n_entries is None else n_entries, n_groups, ptr(counts), ptr(info), n_seqs if capacity is None else capacity)
        assert guards_hold(counts, info)
        return rc, (counts[:-1], info[:-1])

    def associate(self, b, n_seqs, g, n_groups):
        rc, out = self.associate_rc(b, n_seqs, g, n_groups)
        assert rc == 0, self.raw.err()
        return out

    def classify(self, b, n_seqs, g, n_groups):
        rec = np.zeros(n_seqs, CR.DTYPE)
        self.lib.check(self.L.bigsi_hip_classify_batch(b, ptr(g), g.size, n_groups, ptr(rec), n_seqs))
        return rec

    def stream_rc(self, seqs, thr, g, n_groups, k=T.K, handle=None, n_entries=None):
        blob, off = self.lib.pack_seqs(seqs)
        counts, info = preset(len(seqs), max(n_groups, 1))
        rc = self.L.bigsi_hip_associate_stream(handle or self.ix, blob, ptr(off), len(seqs), k, float(thr), ptr(g), g.size if n_entries is None else n_entries, n_groups,
                                               ptr(counts), ptr(info))
        assert guards_hold(counts, info)
        return rc, (counts[:-1], info[:-1])

    def stream(self, seqs, thr, g, n_groups, k=T.K, handle=None):
        rc, out = self.stream_rc(seqs, thr, g, n_groups, k, handle)
        assert rc == 0, self.raw.err()
        return out

    def close(self):
        self.raw.close()


def zeros(n, n_groups):
    return np.zeros((n, n_groups), np.uint32), np.zeros(n, R.INFO_DTYPE)


def check_planted(p, what, thresholds=None, layouts=R.LAYOUTS):
    """one batch of all queries at the three thresholds -- 1.0 is an exact run, the others counting runs, dense and hits-only -- under
    every layout"""
    d = Dev.planted(p)
    b = d.batch(p.seqs)
    n = len(p.seqs)
    try:
        for thr in thresholds or R.thresholds(p):
            for flags in ((SKIP_COMPACT,) if thr == 1.0 else (SKIP_COMPACT, SKIP_COMPACT | SPARSE_COUNTS)):
                d.run(b, thr, flags)
                assert d.info(b).exact == (1 if thr == 1.0 else 0)
                for name in layouts:
                    g, n_groups = R.layout(name, p.n_cols)
                    same(d.associate(b, n, g, n_groups), R.planted_counts(p, thr, name), (what, thr, flags, name))
    finally:
        d.free(b)
        d.close()


@pytest.mark.parametrize("n_cols", WIDTHS)
def test_width_edges(n_cols):
    p = width_case(n_cols)
    if n_cols not in R.CONDITION_WIDTHS:
        assert len(p.seqs) == 5
    check_planted(p, ("width", n_cols))


@pytest.mark.parametrize("n_seqs", sorted(set(QUERY_COUNTS)))
def test_query_counts(n_seqs):
    assert {R.QUERIES - 1, R.QUERIES, R.QUERIES + 1} <= set(QUERY_COUNTS)
    check_planted(T.planted(200, n_seqs, seed=n_seqs), ("queries", n_seqs), layouts=("two", "full64"))


@pytest.mark.parametrize("n_cols", R.CONDITION_WIDTHS)
def test_hit_dense(n_cols):
    check_planted(R.dense_case(n_cols), ("dense", n_cols), thresholds=(1.0, 0.0))


# --------------------------------------------------------------------------------------------- group counts
def groups_layout(n_cols, n_groups):
    """every fifth column in no group, the others dealt round over the groups -- from three groups on over all but the last, which has
    no member"""
    c = np.arange(n_cols)
    g = (c % (n_groups - 1 if n_groups >= 3 else n_groups)).astype(np.uint32)
    g[c % 5 == 0] = R.NONE
    return g


def test_group_counts():
    p = width_case(200)
    thr = p.edge_threshold()[0]
    d = Dev.planted(p)
    n = len(p.seqs)
    b = d.batch(p.seqs)
    GB = R.GROUP_BLOCK
    try:
        for x in (1.0, thr, 0.0):
            d.run(b, x, SKIP_COMPACT if x == 1.0 else SKIP_COMPACT | SPARSE_COUNTS)
            for n_groups in (1, 2, GB - 1, GB, GB + 1, 63, 64):
                g = groups_layout(200, n_groups)
                want = R.group_counts_of(p.us, p.counts, x, g, n_groups)
                assert n_groups < 3 or (R.sizes_of(g, n_groups)[-1] == 0 and not want[0][:, -1].any())          # a group without members counts 0
                assert x != 0.0 or (want[0][p.us > 0] == R.sizes_of(g, n_groups)[None, :]).all()
                same(d.associate(b, n, g, n_groups), want, ("groups", x, n_groups))
            # no column in any group: zeros, with samples_hit still right
            nobody = np.full(200, R.NONE, np.uint32)
            want = R.group_counts_of(p.us, p.counts, x, nobody, 3)
            assert not want[0].any() and not want[1]["grouped_hit"].any() and want[1]["samples_hit"].any()
            same(d.associate(b, n, nobody, 3), want, ("no group", x))
        g = groups_layout(200, 64)
        for bad in (0, 65):
            rc, out = d.associate_rc(b, n, g, bad)
            assert rc == ERR_INVALID and untouched(out) and b"BIGSI_ASSOCIATE_MAX_GROUPS" in d.raw.err()
            rc, out = d.stream_rc(p.seqs, 1.0, g, bad)
            assert rc == ERR_INVALID and untouched(out) and b"BIGSI_ASSOCIATE_MAX_GROUPS" in d.raw.err()
    finally:
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- the classifier on the same run
def test_agrees_with_the_classifier_on_the_same_run():
    for p in (width_case(775), R.dense_case(200)):
        d = Dev.planted(p)
        n = len(p.seqs)
        b = d.batch(p.seqs)
        try:
            for x in ((1.0, 0.0) if p is not width_case(775) else R.thresholds(p)):
                d.run(b, x, SKIP_COMPACT if x == 1.0 else SKIP_COMPACT | SPARSE_COUNTS)
                for name in R.LAYOUTS:
                    g, n_groups = R.layout(name, p.n_cols)
                    counts, info = d.associate(b, n, g, n_groups)
                    rec = d.classify(b, n, g, n_groups)
                    assert np.array_equal(rec["groups_hit"], (counts > 0).sum(axis=1)) and np.array_equal(rec["samples_hit"], info["grouped_hit"])
                    assert np.array_equal(rec["num_unique"], info["num_unique"]) and np.array_equal(rec["min_kmers"], info["min_kmers"])
                    for place in ("best", "second"):
                        there = rec[place + "_group"] != CR.NONE
                        rows = np.flatnonzero(there)
                        assert np.array_equal(rec[place + "_samples_hit"][there], counts[rows, rec[place + "_group"][there]])
                        assert not rec[place + "_samples_hit"][~there].any()
                    assert (rec["best_group"] != CR.NONE).any()
        finally:
            d.free(b)
            d.close()


# --------------------------------------------------------------------------------------------- ordering
def test_associate_reload_run_associate_without_a_wait():
    p = T.planted(200, 65, seed=65)
    thr = p.edge_threshold()[0]
    first, rest = slice(0, 23), slice(23, None)
    g, n_groups = R.layout("two", 200)
    d = Dev.planted(p)
    b = d.batch(p.seqs[first])
    try:
        for x in (1.0, thr):
            want = R.planted_counts(p, x, "two")
            d.run(b, x)
            same(d.associate(b, 23, g, n_groups), part(want, first), ("first", x))
            d.reload(b, p.seqs[rest])          # at once: no wait of the caller's in between
            d.run(b, x)
            same(d.associate(b, 42, g, n_groups), part(want, rest), ("reloaded", x))
            same(d.associate(b, 42, g, n_groups), part(want, rest), ("associated twice", x))
            d.reload(b, p.seqs[first])
        # a batch destroyed right behind its association
        b3 = d.batch(p.seqs[rest])
        d.run(b3, thr)
        out = d.associate(b3, 42, g, n_groups)
        d.free(b3)
        same(out, part(R.planted_counts(p, thr, "two"), rest), "destroy behind associate")
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
        for name in ("two", "full64"):
            g, n_groups = R.layout(name, 200)
            for x in (1.0, p.edge_threshold()[0]):
                want = R.planted_counts(p, x, name)
                assert want[0][:5].any() and want[0][6:].any() and (x == 1.0 or want[0][5].any())          # every chunk has counts to get wrong
                got = d.stream(p.seqs, x, g, n_groups)
                same(got, want, ("stream", name, x))
                again = d.stream(p.seqs, x, g, n_groups)
                assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()          # two calls in a row: bit-identical
        # the batch call over another split gives the same
        for sel in (slice(0, 3), slice(3, 5), slice(6, None)):
            b = d.batch(p.seqs[sel])
            d.run(b, 1.0)
            same(d.associate(b, len(p.seqs[sel]), g, n_groups), part(R.planted_counts(p, 1.0, name), sel), ("batches", sel))
            d.free(b)
        # a call of nothing but short sequences never reaches the device; nor does such a chunk between two that do
        short = ["ACGT", "", "TTTTTTTT"]
        same(d.stream(short, 1.0, g, n_groups), zeros(3, n_groups), "short only")
        filler = ["ACGTACGTAC"] * 4096                              # a whole chunk (4096 sequences) without a k-mer position
        seqs = filler[:4091] + p.seqs[:5] + filler + p.seqs[6:]
        assert T.plan_tally_chunks([len(s) for s in seqs], T.K, 4, 0) == [0, 4096, 8192, 8198]
        got = d.stream(seqs, 1.0, g, n_groups)
        want = R.planted_counts(p, 1.0, name)
        same(part(got, slice(0, 4091)), zeros(4091, n_groups), "the short head of a mixed chunk")
        same(part(got, slice(4091, 4096)), part(want, slice(0, 5)), "behind the short head")
        same(part(got, slice(4096, 8192)), zeros(4096, n_groups), "the chunk of short sequences")
        same(part(got, slice(8192, None)), part(want, slice(6, None)), "behind the chunk of short sequences")
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
    counts, info = zeros(5, n_groups)
    tail = (ptr(counts), ptr(info))
    try:
        # NULL arguments
        for rc in (L.bigsi_hip_associate_batch(None, ptr(g), 65, n_groups, *tail, 5), L.bigsi_hip_associate_batch(b, None, 65, n_groups, *tail, 5),
                   L.bigsi_hip_associate_batch(b, ptr(g), 65, n_groups, None, ptr(info), 5), L.bigsi_hip_associate_batch(b, ptr(g), 65, n_groups, ptr(counts), None, 5),
                   L.bigsi_hip_associate_stream(None, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, *tail),
                   L.bigsi_hip_associate_stream(d.ix, blob, None, 5, T.K, 1.0, ptr(g), 65, n_groups, *tail),
                   L.bigsi_hip_associate_stream(d.ix, blob, ptr(off), 5, T.K, 1.0, None, 65, n_groups, *tail),
                   L.bigsi_hip_associate_stream(d.ix, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, None, ptr(info)),
                   L.bigsi_hip_associate_stream(d.ix, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, ptr(counts), None),
                   L.bigsi_hip_associate_stream(d.ix, None, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, *tail)):
            assert rc == ERR_INVALID and d.raw.err()
        # what a stream's arguments are refused for: outputs untouched
        down = off.copy()
        down[2] = down[1] - 1
        for n, k, x, o in ((0, T.K, 1.0, off), (5, 0, 1.0, off), (5, T.K, 1.5, off), (5, T.K, float("nan"), off), (5, T.K, 1.0, down)):
            out = preset(5, n_groups)
            assert L.bigsi_hip_associate_stream(d.ix, blob, ptr(o), n, k, x, ptr(g), 65, n_groups, ptr(out[0]), ptr(out[1])) == ERR_INVALID and untouched(out)
        # group_of: its length, n_groups, a value out of range (the column is named) -- batch and stream alike
        d.run(b, 1.0)
        bad = g.copy()
        bad[64] = n_groups
        for gg, n_entries, groups, word in ((g, 64, n_groups, b"64 entries"), (g, 66, n_groups, b"66 entries"), (g, None, 0, b"BIGSI_ASSOCIATE_MAX_GROUPS"),
                                            (g, None, 65, b"BIGSI_ASSOCIATE_MAX_GROUPS"), (bad, None, n_groups, b"group_of[64]"), (g, None, 7, b"group_of[64]")):
            rc, out = d.associate_rc(b, 5, gg, groups, n_entries=n_entries)
            assert rc == ERR_INVALID and untouched(out) and word in d.raw.err(), (n_entries, groups, d.raw.err())
            rc, out = d.stream_rc(p.seqs, 1.0, gg, groups, n_entries=n_entries)
            assert rc == ERR_INVALID and untouched(out) and word in d.raw.err()
        # capacity: nothing written
        rc, out = d.associate_rc(b, 5, g, n_groups, capacity=4)
        assert rc == ERR_CAPACITY and untouched(out)
        # a batch that has not run; one whose run built hit lists
        fresh = d.batch(p.seqs)
        rc, out = d.associate_rc(fresh, 5, g, n_groups)
        assert rc == ERR_STATE and untouched(out) and b"not completed" in d.raw.err()
        d.free(fresh)
        for thr in (1.0, 0.5):
            d.run(b, thr, flags=0)
            rc, out = d.associate_rc(b, 5, g, n_groups)
            assert rc == ERR_STATE and untouched(out) and b"an association takes a run made with BIGSI_RUN_SKIP_COMPACT" in d.raw.err()
        # a result limit, caller-owned bit vectors, a result width
        d.run(b, 1.0)
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 5, None, 0))
        rc, out = d.associate_rc(b, 5, g, n_groups)
        assert rc == ERR_STATE and untouched(out) and b"limit" in d.raw.err() and b"an association counts every hit" in d.raw.err()
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 0, None, 0))
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, C.c_void_p(d.info(b).d_bitmaps)))
        rc, out = d.associate_rc(b, 5, g, n_groups)
        assert rc == ERR_STATE and untouched(out)
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, None))
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 64))
        rc, out = d.associate_rc(b, 5, g, n_groups)
        assert rc == ERR_STATE and untouched(out)
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 0))
        # num_hashes changed since the run
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, 2))
        rc, out = d.associate_rc(b, 5, g, n_groups)
        assert rc == ERR_STATE and untouched(out) and b"num_hashes" in d.raw.err()
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, T.H))
        # num_cols changed since the run: 64 columns are one result word fewer than the batch's vectors have
        d.lib.check(L.bigsi_hip_set_num_cols(d.ix, 64))
        rc, out = d.associate_rc(b, 5, g[:64].copy(), n_groups)
        assert rc == ERR_STATE and untouched(out) and b"num_cols changed" in d.raw.err()
        d.lib.check(L.bigsi_hip_set_num_cols(d.ix, 65))
        # ... and the batch is fine
        same(d.associate(b, 5, g, n_groups), R.planted_counts(p, 1.0, "edges"), "after the refusals")
        # an index without columns
        empty = Raw(64, 0, cap=8, h=3)
        rc = L.bigsi_hip_associate_stream(empty.ix, blob, ptr(off), 5, T.K, 1.0, ptr(g), 0, n_groups, *tail)
        assert rc == ERR_STATE
        empty.close()
    finally:
        d.free(b)
        d.close()


def test_view_handle():
    p = T.planted(129, 5)
    thr = p.edge_threshold()[0]
    g, n_groups = R.layout("full64", 129)
    d = Dev.planted(p)
    view = C.c_void_p()
    d.lib.check(d.L.bigsi_hip_open_view(d.ix, C.byref(view)))
    b = d.batch(p.seqs, handle=view)
    try:
        for x in (1.0, thr):
            d.run(b, x)
            same(d.associate(b, 5, g, n_groups), R.planted_counts(p, x, "full64"), ("view, batch", x))
            same(d.stream(p.seqs, x, g, n_groups, handle=view), R.planted_counts(p, x, "full64"), ("view, stream", x))
    finally:
        d.free(b)
        d.lib.check(d.L.bigsi_hip_close(view))
        d.close()


# --------------------------------------------------------------------------------------------- end to end
KB, MB, HB = 11, 100003, 3


def test_bigsi_associate_and_command_line(tmp_path, capsys):
    """BIGSI.associate and `associate` on an index built from sequences, one sample deleted, with and without --others: the result, the
    TSV and the JSON are the host layer's (bigsi_amd/associate.py) for the numpy reference over the samples' own Bloom filters."""
    from bigsi_amd import BIGSI, associate
    from bigsi_amd.__main__ import main
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(41)
    probe, other = rand_seq(rng, 60), rand_seq(rng, 50)
    seqs = {"s0": rand_seq(rng, 200), "s1": rand_seq(rng, 100) + probe + rand_seq(rng, 60), "s2": rand_seq(rng, 300) + other, "s3": probe + rand_seq(rng, 150),
            "s4": rand_seq(rng, 90) + probe[:40] + other, "s5": rand_seq(rng, 250)}
    cfg = {"storage-engine": "hip-hbm", "k": KB, "m": MB, "h": HB, "storage-config": {"name": "associate%d" % next(_counter), "filename": str(tmp_path / "index.hbm")}}
    b = BIGSI.build_from_sequences(cfg, {n: [s] for n, s in seqs.items()})
    try:
        b.delete_sample("s3")
        queries = [probe, other, "ACGT", probe[5:45], rand_seq(rng, 70), seqs["s5"][20:90], other[:30] + probe[:30]]
        filters = np.stack([np.unpackbits(np.frombuffer(BIGSI.bloom(cfg, list(seq_to_kmers(s, KB))).tobytes(), dtype=np.uint8))[:MB] for s in seqs.values()], axis=1)
        dense = np.packbits(filters, axis=1)
        pairs = [T.counts_of(dense, 6, HB, q, KB) for q in queries]
        us, counts = [u for u, _ in pairs], np.stack([c for _, c in pairs])
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
            sizes = R.sizes_of(g, len(gn))
            assert sizes.tolist() == ([2, 1] if others is None else [2, 1, 2])          # the deleted s3 is in no group and in no size
            for thr, min_af in ((1.0, None), (0.6, None), (0.6, 0.3)):
                ref = R.group_counts_of(us, counts, thr, g, len(gn))
                want = associate.result(ref[0], ref[1], gn, sizes, min_af)
                got = b.associate(queries, groups, threshold=thr, others=others, min_af=min_af)
                assert got == want, (others, thr, min_af)
                assert b.associate(iter(queries), {"P": ["s1", "s4"], "O": ["s2"]}, threshold=thr, others=others, min_af=min_af) == want
                chunks = list(b.associate_arrays(queries, groups, threshold=thr, others=others, batch_kmers=4))          # many small slices
                assert len(chunks) > 1 and [s for c, _, _ in chunks for s in c] == queries
                same((np.concatenate([c for _, c, _ in chunks]), np.concatenate([i for _, _, i in chunks])), ref, ("slices", others, thr))
                capsys.readouterr()
                argv = ["associate", str(fa), "--groups", str(group_file), "-t", str(thr), "--config", str(cf)] + (["--others", others] if others else []) + \
                    (["--min-af", str(min_af)] if min_af is not None else [])
                assert main(argv) == 0
                assert capsys.readouterr().out == associate.to_tsv(want, ids) + "\n"
                assert main(argv + ["--format", "json"]) == 0
                assert capsys.readouterr().out == associate.to_json(want, ids) + "\n"
            res = b.associate(queries, groups, threshold=0.6, others=others, min_af=0.3)
            assert res["dropped"] > 0 and len(res["records"]) + res["dropped"] == len(queries) and res["records"]
        res = b.associate(queries, groups, threshold=1.0)
        assert res["records"][0]["groups"]["P"]["hit"] == 1 and res["records"][0]["groups"]["O"]["hit"] == 0          # the probe: whole in s1 (s3 is deleted)
        assert res["records"][1]["groups"]["P"]["hit"] == 1 and res["records"][1]["groups"]["O"]["hit"] == 1          # `other` is whole in s2 and s4
        assert res["records"][2]["num_kmers"] == 0 and res["records"][0]["samples_hit"] >= 2                          # the deleted s3's column still holds the probe
        assert b.associate([], groups) == {"groups": ["P", "O"], "sizes": [2, 1], "total": 3, "records": [], "dropped": 0}
        with pytest.raises(KeyError):
            b.associate(queries, [("s3", "P")])                      # a deleted sample cannot be listed
    finally:
        b.delete()
