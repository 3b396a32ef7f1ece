"""The query-set tally on the device (include/bigsi_hip_tally.h), straight on the C ABI: k_tally_hits in its three instances
(<uint16_t, EXACT>, <uint16_t>, <uint32_t>) and k_tally_totals against numpy -- oracle.coracle's hashing plus the row bytes
(tests/tally_ref.py, count_staircase's reference()), never a library call -- on indexes written by bigsi_hip_set_rows with junk bits
behind num_cols.  Width edges (hits planted in column 0, 63, 64, the first and the last column of the last word, at threshold 1 and
at a threshold whose min_kmers sits exactly on a count an edge column holds), query tiles around plan_tally's tile, both counter
widths and the k_count_combine route on the staircase cases, accumulation over batches, reset, fetch twice, add / reload / run / add
without a wait in between, add_stream over three chunks (one of them a single sequence of 2^20 + 200 positions) against the one-batch
reference and against add_batch over another split, every refusal, a view handle, and BIGSI.tally / `python -m bigsi_amd tally` end
to end with a deleted sample.  tests/test_tally_host.py asserts, on the CPU, that none of the references is vacuous."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import yaml

import tally_ref as T
from count_staircase import K as SK, build_case, min_kmers
from raw_index import Raw, ptr, rand_seq
from test_tally_host import TILE_SEQS, WIDTHS

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

    def tally(self, handle=None):
        t = C.c_void_p()
        self.lib.check(self.L.bigsi_hip_tally_create(handle or self.ix, C.byref(t)))
        return t

    def add(self, t, b):
        self.lib.check(self.L.bigsi_hip_tally_add_batch(t, b))

    def add_stream(self, t, seqs, thr, k=T.K):
        blob, off = self.lib.pack_seqs(seqs)
        self.lib.check(self.L.bigsi_hip_tally_add_stream(t, blob, ptr(off), len(seqs), k, float(thr)))

    def fetch_rc(self, t, capacity=None):
        """(rc, queries_hit, kmers_found, totals) over buffers preset to a pattern, with a guard entry behind num_cols"""
        n = self.n_cols
        qh, kf, totals = np.full(n + 1, 0xAB, np.uint64), np.full(n + 1, 0xAB, np.uint64), np.full(4, 0xAB, np.uint64)
        rc = self.L.bigsi_hip_tally_fetch(t, ptr(qh), ptr(kf), n if capacity is None else capacity, ptr(totals))
        assert qh[n] == 0xAB and kf[n] == 0xAB
        return rc, qh[:n], kf[:n], totals

    def fetch(self, t):
        rc, qh, kf, totals = self.fetch_rc(t)
        assert rc == 0, self.raw.err()
        return qh, kf, totals

    def reset(self, t):
        self.lib.check(self.L.bigsi_hip_tally_reset(t))

    def drop(self, t):
        self.lib.check(self.L.bigsi_hip_tally_destroy(t))

    def close(self):
        self.raw.close()


def same(got, want, what):
    for name, g, w in zip(("queries_hit", "kmers_found", "totals"), got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])


def check_planted(p, what):
    """one batch of all queries, at threshold 1 (the EXACT instance) and at the edge threshold (counters), on one tally that is reset"""
    thr = p.edge_threshold()[0]
    d = Dev.planted(p)
    b, t = d.batch(p.seqs), d.tally()
    try:
        for x in (1.0, thr, 1.0):
            d.run(b, x)
            assert d.info(b).exact == (1 if x == 1.0 else 0)
            d.add(t, b)
            same(d.fetch(t), p.tally(x), (what, x))
            d.reset(t)
        d.run(b, thr, flags=SKIP_COMPACT | SPARSE_COUNTS)          # hits-only counters: a word that holds a hit keeps all 64 of its counters
        d.add(t, b)
        same(d.fetch(t), p.tally(thr), (what, thr, "sparse counters"))
    finally:
        d.drop(t)
        d.free(b)
        d.close()


@pytest.mark.parametrize("n_cols", WIDTHS)
def test_width_edges(n_cols):
    check_planted(T.planted(n_cols, 9), ("width", n_cols))


@pytest.mark.parametrize("n_seqs", TILE_SEQS)
def test_query_tiles(n_seqs):
    check_planted(T.planted(200, n_seqs, seed=n_seqs), ("tile", n_seqs))


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
    rows = np.random.default_rng(3).integers(0, 256, size=(sc.row_ids.size, stride), dtype=np.uint8)          # junk behind num_cols (200 and 400: whole bytes)
    assert c["n_cols"] % 8 == 0
    rows[:, :sc.packed.shape[1]] = sc.packed
    d = Dev(c["m"], c["n_cols"], c["h"], sc.row_ids, rows)
    b, t = d.batch(queries, SK), d.tally()
    try:
        for thr in sc.thresholds + [0.0]:
            d.run(b, thr)
            inf = d.info(b)
            assert inf.exact == 0 and inf.count_bytes == count_bytes == c["route"]["count_bytes"], (name, thr)
            d.add(t, b)
            got, want = d.fetch(t), T.tally_of(us, counts, thr)
            same(got, want, (name, thr))
            if thr == 0.0:          # every sample is hit by every counted query
                assert (got[0] == int((us > 0).sum())).all() and np.array_equal(got[1], counts[us > 0].sum(axis=0).astype(np.uint64))
            else:
                assert min_kmers(sc.u, thr) in counts[0] and got[0].max() >= 1          # a column of the main query sits exactly on min_kmers
            d.reset(t)
    finally:
        d.drop(t)
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- accumulation and ordering
def test_accumulation_reset_and_reload():
    p = T.planted(200, 65, seed=65)
    thr = p.edge_threshold()[0]
    first, rest = slice(0, 23), slice(23, None)
    d = Dev.planted(p)
    b1, b2, t = d.batch(p.seqs[first]), d.batch(p.seqs[rest]), d.tally()
    try:
        zero = (np.zeros(200, np.uint64), np.zeros(200, np.uint64), np.zeros(4, np.uint64))
        same(d.fetch(t), zero, "a new tally")
        for x in (1.0, thr):
            # two batches = one reference over both
            d.run(b1, x)
            d.run(b2, x)
            d.add(t, b1)
            same(d.fetch(t), p.tally(x, first), ("one of two", x))
            d.add(t, b2)
            same(d.fetch(t), p.tally(x), ("two batches", x))
            same(d.fetch(t), p.tally(x), ("fetch twice", x))
            d.add(t, b1)          # the same batch again counts again
            same(d.fetch(t), T.add(p.tally(x), p.tally(x, first)), ("added twice", x))
            d.reset(t)
            same(d.fetch(t), zero, ("reset", x))
            # add, at once reload the same batch with other queries, run, add: no wait of the caller's in between
            d.add(t, b1)
            d.reload(b1, p.seqs[rest])
            d.run(b1, x)
            d.add(t, b1)
            d.reload(b1, p.seqs[first])
            same(d.fetch(t), p.tally(x), ("add / reload / run / add", x))
            d.reset(t)
        # thresholds mix in one tally: the sums add up
        d.run(b1, 1.0)
        d.add(t, b1)
        d.run(b1, thr)
        d.add(t, b1)
        same(d.fetch(t), T.add(p.tally(1.0, first), p.tally(thr, first)), "two thresholds")
        # a batch destroyed right behind its add
        d.reset(t)
        b3 = d.batch(p.seqs[rest])
        d.run(b3, thr)
        d.add(t, b3)
        d.free(b3)
        same(d.fetch(t), p.tally(thr, rest), "destroy behind add")
    finally:
        d.drop(t)
        d.free(b1)
        d.free(b2)
        d.close()


def test_add_stream_over_three_chunks():
    lengths = T.stream_lengths()
    p = T.planted(200, len(lengths), seed=12, lengths=lengths)
    assert T.plan_tally_chunks([len(s) for s in p.seqs], T.K, 4, 4) == [0, 5, 6, 12] and p.us[5] > (1 << 19)
    thr = p.edge_threshold()[0]
    d = Dev.planted(p)
    t, t2 = d.tally(), d.tally()
    try:
        for x in (1.0, thr):
            d.add_stream(t, p.seqs, x)
            got = d.fetch(t)
            same(got, p.tally(x), ("stream", x))
            # ... and equals add_batch over another split
            for part in (slice(0, 3), slice(3, None)):
                b = d.batch(p.seqs[part])
                d.run(b, x)
                d.add(t2, b)
                d.free(b)
            same(d.fetch(t2), got, ("stream against batches", x))
            # a second stream call adds to the first; one of nothing but short sequences counts them as skipped
            d.add_stream(t, p.seqs[:5], x)
            d.add_stream(t, ["ACGT", "", "TTTTTTTT"], x)
            want = T.add(p.tally(x), p.tally(x, slice(0, 5)))
            want[2][2] += 3
            same(d.fetch(t), want, ("two streams", x))
            d.reset(t)
            d.reset(t2)
    finally:
        d.drop(t)
        d.drop(t2)
        d.close()


# --------------------------------------------------------------------------------------------- refusals
def test_refusals():
    p = T.planted(65, 9)
    d, other = Dev.planted(p), Dev.planted(p)
    L = d.L
    b, t = d.batch(p.seqs), d.tally()
    foreign = other.batch(p.seqs)
    blob, off = d.lib.pack_seqs(p.seqs)
    try:
        out, tot, h = np.zeros(65, np.uint64), np.zeros(4, np.uint64), C.c_void_p()
        # NULL arguments
        for rc in (L.bigsi_hip_tally_create(None, C.byref(h)), L.bigsi_hip_tally_create(d.ix, None), L.bigsi_hip_tally_reset(None),
                   L.bigsi_hip_tally_add_batch(None, b), L.bigsi_hip_tally_add_batch(t, None),
                   L.bigsi_hip_tally_add_stream(None, blob, ptr(off), 9, T.K, 1.0), L.bigsi_hip_tally_add_stream(t, blob, None, 9, T.K, 1.0),
                   L.bigsi_hip_tally_fetch(None, ptr(out), ptr(out), 65, ptr(tot)), L.bigsi_hip_tally_fetch(t, None, ptr(out), 65, ptr(tot)),
                   L.bigsi_hip_tally_fetch(t, ptr(out), None, 65, ptr(tot)), L.bigsi_hip_tally_fetch(t, ptr(out), ptr(out), 65, None)):
            assert rc == ERR_INVALID and d.raw.err()
        assert L.bigsi_hip_tally_destroy(None) == 0
        # what a batch's arguments are refused for
        for n, k, x in ((0, T.K, 1.0), (9, 0, 1.0), (9, T.K, 1.5), (9, T.K, float("nan"))):
            assert L.bigsi_hip_tally_add_stream(t, blob, ptr(off), n, k, x) == ERR_INVALID
        # a batch that has not run; one of another index; one whose run built hit lists
        assert L.bigsi_hip_tally_add_batch(t, b) == ERR_STATE and b"not completed" in d.raw.err()
        other.run(foreign, 1.0)
        assert L.bigsi_hip_tally_add_batch(t, foreign) == ERR_STATE and b"another index" in d.raw.err()
        for thr in (1.0, 0.5):
            d.run(b, thr, flags=0)
            assert L.bigsi_hip_tally_add_batch(t, b) == ERR_STATE and b"SKIP_COMPACT" in d.raw.err()
        # a result limit, caller-owned bit vectors, a result width
        d.run(b, 1.0)
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 5, None, 0))
        assert L.bigsi_hip_tally_add_batch(t, b) == ERR_STATE and b"limit" in d.raw.err()
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 0, None, 0))
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, C.c_void_p(d.info(b).d_bitmaps)))
        assert L.bigsi_hip_tally_add_batch(t, b) == ERR_STATE
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, None))
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 64))
        assert L.bigsi_hip_tally_add_batch(t, b) == ERR_STATE
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 0))
        same(d.fetch(t), (np.zeros(65, np.uint64), np.zeros(65, np.uint64), np.zeros(4, np.uint64)), "refused calls added nothing")
        d.add(t, b)          # ... and the batch is fine
        same(d.fetch(t), p.tally(1.0), "after the refusals")
        # capacity: outputs untouched
        rc, qh, kf, totals = d.fetch_rc(t, capacity=64)
        assert rc == ERR_CAPACITY and (qh == 0xAB).all() and (kf == 0xAB).all() and (totals == 0xAB).all()
        # the index changed under the tally: num_cols, then num_hashes
        d.lib.check(L.bigsi_hip_set_num_cols(d.ix, 64))
        assert L.bigsi_hip_tally_add_batch(t, b) == ERR_STATE and d.fetch_rc(t)[0] == ERR_STATE and L.bigsi_hip_tally_reset(t) == ERR_STATE
        assert L.bigsi_hip_tally_add_stream(t, blob, ptr(off), 9, T.K, 1.0) == ERR_STATE and b"changed" in d.raw.err()
        # ... and under the batch: a tally made now is refused the batch that ran at 65 columns, and nothing is added to it
        t64 = d.tally()
        try:
            assert L.bigsi_hip_tally_add_batch(t64, b) == ERR_STATE and b"num_cols changed" in d.raw.err()
            rc, qh, kf, totals = d.fetch_rc(t64)
            assert rc == 0 and not qh[:64].any() and not kf[:64].any() and not totals.any()
        finally:
            d.drop(t64)
        d.lib.check(L.bigsi_hip_set_num_cols(d.ix, 65))
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, 2))
        assert L.bigsi_hip_tally_add_batch(t, b) == ERR_STATE and d.fetch_rc(t)[0] == ERR_STATE
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, T.H))
        same(d.fetch(t), p.tally(1.0), "the index as it was")
    finally:
        d.drop(t)
        d.free(b)
        other.free(foreign)
        d.close()
        other.close()


def test_view_handle():
    p = T.planted(129, 9)
    thr = p.edge_threshold()[0]
    d = Dev.planted(p)
    view = C.c_void_p()
    d.lib.check(d.L.bigsi_hip_open_view(d.ix, C.byref(view)))
    t, b, own = d.tally(view), d.batch(p.seqs, handle=view), d.batch(p.seqs)
    try:
        d.run(own, 1.0)
        assert d.L.bigsi_hip_tally_add_batch(t, own) == ERR_STATE          # the owner's batch is a batch of another handle
        for x in (1.0, thr):
            d.run(b, x)
            d.add(t, b)
            same(d.fetch(t), p.tally(x), ("view, batch", x))
            d.reset(t)
            d.add_stream(t, p.seqs, x)
            same(d.fetch(t), p.tally(x), ("view, stream", x))
            d.reset(t)
    finally:
        d.drop(t)
        d.free(b)
        d.free(own)
        d.lib.check(d.L.bigsi_hip_close(view))
        d.close()


# --------------------------------------------------------------------------------------------- end to end
KB, MB, HB = 11, 100003, 3


def test_bigsi_tally_and_command_line(tmp_path, capsys):
    """BIGSI.tally and `tally` on an index built from sequences, one sample deleted: the record, the JSON and the CSV are the host
    layer's (bigsi_amd/tally.py) for the numpy reference over the samples' own Bloom filters."""
    from bigsi_amd import BIGSI, tally
    from bigsi_amd.__main__ import main
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(41)
    probe, other = rand_seq(rng, 60), rand_seq(rng, 50)
    seqs = {"s0": rand_seq(rng, 200), "s1": rand_seq(rng, 100) + probe + rand_seq(rng, 60), "s2": rand_seq(rng, 300) + other, "s3": probe + rand_seq(rng, 150),
            "s4": rand_seq(rng, 90) + probe[:40] + other, "s5": rand_seq(rng, 250)}
    cfg = {"storage-engine": "hip-hbm", "k": KB, "m": MB, "h": HB, "storage-config": {"name": "tally%d" % next(_counter), "filename": str(tmp_path / "index.hbm")}}
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
        for thr in (1.0, 0.6):
            qh, kf, totals = T.tally_of(us, counts, thr)
            want = tally.record(qh, kf, totals, names.__getitem__, excluded=[3])
            assert qh[3] >= 2 and [r["colour"] for r in want["samples"]].count(3) == 0 and len(want["samples"]) >= 3 and want["skipped"] == 1
            assert b.tally(queries, threshold=thr) == want
            assert b.tally(iter(queries), threshold=thr, limit=2) == dict(want, samples=want["samples"][:2])
            assert b.tally(queries, threshold=thr, batch_kmers=4) == want          # many small slices
        assert b.tally([]) == {"queries": 0, "kmers": 0, "skipped": 0, "queries_with_hits": 0, "samples": []}
        # the command, on the index's snapshot
        b.storage.sync()
        cf, fa = tmp_path / "config.yaml", tmp_path / "q.fa"
        cf.write_text(yaml.safe_dump(cfg))
        fa.write_text("".join(">q%d\n%s\n" % (i, q) for i, q in enumerate(queries)))
        capsys.readouterr()
        for thr in (1.0, 0.6):
            want = tally.record(*T.tally_of(us, counts, thr), names.__getitem__, excluded=[3])
            assert main(["tally", str(fa), "-t", str(thr), "--config", str(cf)]) == 0
            assert capsys.readouterr().out == tally.to_json(want) + "\n"
            assert main(["tally", str(fa), "-t", str(thr), "--limit", "2", "--format", "csv", "--config", str(cf)]) == 0
            assert capsys.readouterr().out == tally.to_csv(dict(want, samples=want["samples"][:2])) + "\n"
        assert json.loads(tally.to_json(want))["samples"][0]["queries_hit"] >= 2
    finally:
        b.delete()
