"""Locus typing on the device (include/bigsi_hip_typing.h), straight on the C ABI: k_locus_best in its three instances (<uint16_t,
EXACT>, <uint16_t>, <uint32_t>) and k_locus_counts against numpy -- oracle.coracle's hashing plus the row bytes (tests/typing_ref.py
over tally_ref's planted indexes), never a library call -- on indexes written by bigsi_hip_set_rows with junk bits behind num_cols.
Width edges (65, 129 and 775 columns have an odd number of result words: a pad word is there to be misread) under three record
layouts at threshold 1, 0.4, at a threshold whose min_kmers sits exactly on a count an edge column holds and at 0, dense and
hits-only counters, with and without a column selection; both counter widths on the staircase cases; the set cut into two batches
in either order; reset, fetch twice and without cells; add / reload / run / add and destroy-behind-add without a host wait;
add_stream over three chunks (one of them a single sequence of 2^20 + 200 positions); every refusal with preset outputs; the hit
counts against bigsi_hip_search_batch's hit lists; a view handle; and BIGSI.type_samples / `python -m bigsi_amd typing` end to end on
a small built index with a profiles table and a deleted sample.  No tolerance anywhere.  tests/test_typing_host.py asserts, on the
CPU, that none of the references is vacuous."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import yaml

import tally_ref as T
import typing_ref as R
from raw_index import Raw, ptr
from test_typing_host import Out, same

pytestmark = pytest.mark.gpu
_counter = itertools.count()
SKIP_COMPACT, SPARSE_COUNTS = 2, 8
ERR_INVALID, ERR_NOMEM, ERR_CAPACITY, ERR_STATE = -1, -3, -5, -6


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

    def create_rc(self, n_loci, columns=None, handle=None):
        t = C.c_void_p()
        return self.L.bigsi_hip_typing_create(handle or self.ix, n_loci, ptr(columns), C.byref(t)), t

    def create(self, n_loci, columns=None, handle=None):
        rc, t = self.create_rc(n_loci, columns, handle)
        assert rc == 0 and t.value, self.raw.err()
        return t

    def destroy(self, t):
        self.lib.check(self.L.bigsi_hip_typing_destroy(t))

    def reset(self, t):
        self.lib.check(self.L.bigsi_hip_typing_reset(t))

    def add_rc(self, t, b, locus_of, allele_of, n_entries=None):
        locus_of, allele_of = np.ascontiguousarray(locus_of, np.uint32), np.ascontiguousarray(allele_of, np.uint32)
        return self.L.bigsi_hip_typing_add_batch(t, b, ptr(locus_of), ptr(allele_of), locus_of.size if n_entries is None else n_entries)

    def add(self, t, b, locus_of, allele_of):
        assert self.add_rc(t, b, locus_of, allele_of) == 0, self.raw.err()

    def stream_rc(self, t, seqs, thr, locus_of, allele_of, k=T.K):
        blob, off = self.lib.pack_seqs(seqs)
        locus_of, allele_of = np.ascontiguousarray(locus_of, np.uint32), np.ascontiguousarray(allele_of, np.uint32)
        return self.L.bigsi_hip_typing_add_stream(t, blob, ptr(off), len(seqs), k, float(thr), ptr(locus_of), ptr(allele_of))

    def stream(self, t, seqs, thr, locus_of, allele_of):
        assert self.stream_rc(t, seqs, thr, locus_of, allele_of) == 0, self.raw.err()

    def fetch_rc(self, t, n_loci, cells=True, cell_cap=None, sample_cap=None):
        """(rc, Out) over buffers preset to a pattern, with a guard row behind each"""
        out = Out(n_loci, self.n_cols)
        rc = self.L.bigsi_hip_typing_fetch(t, ptr(out.best) if cells else None, ptr(out.hits) if cells else None, n_loci * self.n_cols if cell_cap is None else cell_cap,
                                           ptr(out.loci), ptr(out.samples), self.n_cols if sample_cap is None else sample_cap, ptr(out.records))
        assert out.guards_hold()
        return rc, out

    def fetch(self, t, n_loci, cells=True):
        rc, out = self.fetch_rc(t, n_loci, cells)
        assert rc == 0, self.raw.err()
        if not cells:
            assert out.best.tobytes() == b"\xab" * out.best.nbytes and out.hits.tobytes() == b"\xab" * out.hits.nbytes
        return out.got(cells)

    def close(self):
        self.raw.close()


def runs_of(thr):
    """1.0 is an exact run, the others counting runs, dense and hits-only"""
    return (SKIP_COMPACT,) if thr == 1.0 else (SKIP_COMPACT, SKIP_COMPACT | SPARSE_COUNTS)


def equal(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


# --------------------------------------------------------------------------------------------- widths, layouts, thresholds, selections
@pytest.mark.parametrize("n_cols", R.WIDTHS)
def test_width_edges(n_cols):
    p = R.width_case(n_cols)
    columns = R.column_mask(p)[0]
    d = Dev.planted(p)
    try:
        cells = {}
        for name in R.LAYOUTS:
            order, lo, al, nl = R.layout(name, len(p.seqs))
            b = d.batch([p.seqs[q] for q in order])
            accs = {False: d.create(nl), True: d.create(nl, columns)}
            try:
                for thr in R.thresholds(p):
                    for flags in runs_of(thr):
                        d.run(b, thr, flags)
                        assert d.info(b).exact == (1 if thr == 1.0 else 0)
                        for masked, t in accs.items():
                            d.reset(t)
                            d.add(t, b, lo, al)
                            got = d.fetch(t, nl)
                            same(got, R.planted_typing(p, thr, name, masked), ("width", n_cols, name, thr, flags, masked))
                            cells[(name, thr, flags, masked)] = got
            finally:
                for t in accs.values():
                    d.destroy(t)
                d.free(b)
        # grouped and interleaved are the same scheme in another order: identical cells and counts, bit for bit
        for (name, thr, flags, masked), got in cells.items():
            if name == "grouped":
                assert equal(got, cells[("interleaved", thr, flags, masked)]), (n_cols, thr, flags, masked)
    finally:
        d.close()


# --------------------------------------------------------------------------------------------- counter widths: the staircase cases
@pytest.mark.parametrize("name, count_bytes", [("Uplain10", 2), ("S32", 4), ("S10b", 2)])
def test_counter_widths(name, count_bytes):
    from count_staircase import K as SK, build_case
    c, sc, queries = build_case(name)
    pairs = [sc.reference(q) for q in queries]
    us, counts = np.array([u for u, _ in pairs], np.int64), np.stack([x for _, x in pairs])
    n = len(queries)
    order, lo, al = np.arange(n), (np.arange(n) % 3).astype(np.uint32), (n - np.arange(n)).astype(np.uint32)          # three loci with records, one without
    probe = Raw(c["m"], c["n_cols"], h=c["h"])
    stride = probe.stride
    probe.close()
    rows = np.random.default_rng(3).integers(0, 256, size=(sc.row_ids.size, stride), dtype=np.uint8)          # junk behind num_cols (whole bytes)
    assert c["n_cols"] % 8 == 0
    rows[:, :sc.packed.shape[1]] = sc.packed
    d = Dev(c["m"], c["n_cols"], c["h"], sc.row_ids, rows)
    b, t = d.batch(queries, SK), d.create(4)
    try:
        partial = 0
        for thr in sc.thresholds + [0.0]:
            for flags in (SKIP_COMPACT, SKIP_COMPACT | SPARSE_COUNTS):
                d.run(b, thr, flags)
                inf = d.info(b)
                assert inf.exact == 0 and inf.count_bytes == count_bytes == c["route"]["count_bytes"], (name, thr)
                mk = np.array([T.min_kmers(int(u), thr) for u in us], np.int64)
                want = R.typing_of(us, counts, (counts >= mk[:, None]) & (us > 0)[:, None], order, lo, al, 4)
                d.reset(t)
                d.add(t, b, lo, al)
                same(d.fetch(t, 4), want, (name, thr, flags))
                partial += int(want["loci"][:, 0].sum() - want["loci"][:, 1].sum())
                assert not want["records"][3] and not want["best"][3].any()
        assert partial > 0, "no partial score: the counters were never read"
    finally:
        d.destroy(t)
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- accumulation
def test_two_batches_in_either_order_reset_and_fetch():
    p = R.width_case(200)
    thr = 0.4
    order, lo, al, nl = R.layout("grouped", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    want = R.planted_typing(p, thr, "grouped")
    d = Dev.planted(p)
    whole, first, second = d.batch(seqs), d.batch(seqs[:29]), d.batch(seqs[29:])
    t = d.create(nl)
    try:
        for b in (whole, first, second):
            d.run(b, thr, SKIP_COMPACT | SPARSE_COUNTS)
        assert lo[28] == lo[29]                                          # the cut goes through a locus: both halves feed its cells
        d.add(t, first, lo[:29], al[:29])
        half = d.fetch(t, nl)
        assert not equal(half, want) and half["records"].sum() < want["records"].sum()
        d.add(t, second, lo[29:], al[29:])
        both = d.fetch(t, nl)
        same(both, want, "two halves")
        d.reset(t)
        d.add(t, second, lo[29:], al[29:])
        d.add(t, first, lo[:29], al[:29])
        assert equal(d.fetch(t, nl), both), "the halves in the other order"
        # fetch twice: identical; without cells: the same counts, no cell written
        assert equal(d.fetch(t, nl), both)
        counts_only = d.fetch(t, nl, cells=False)
        assert all(counts_only[k].tobytes() == both[k].tobytes() for k in ("loci", "samples", "records"))
        # the cells keep accumulating behind a fetch: the same records again leave best alone and double hits and records
        d.add(t, whole, lo, al)
        again = d.fetch(t, nl)
        assert again["best"].tobytes() == both["best"].tobytes() and np.array_equal(again["hits"], 2 * want["hits"]) and np.array_equal(again["records"], 2 * want["records"])
        assert np.array_equal(again["loci"][:, :2], want["loci"][:, :2]) and np.array_equal(again["loci"][:, 2], want["loci"][:, 0])          # every called cell now has hits > 1
        # reset zeroes
        d.reset(t)
        zero = d.fetch(t, nl)
        assert not any(zero[k].any() for k in zero)
        d.add(t, whole, lo, al)
        same(d.fetch(t, nl), want, "after reset")
    finally:
        d.destroy(t)
        for b in (whole, first, second):
            d.free(b)
        d.close()


def test_add_reload_run_add_without_a_wait():
    p = R.width_case(200)
    thr = R.thresholds(p)[2]
    order, lo, al, nl = R.layout("shuffled", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    d = Dev.planted(p)
    b = d.batch(seqs[:23])
    t = d.create(nl)
    try:
        for x in (1.0, thr):
            d.reset(t)
            d.run(b, x)
            d.add(t, b, lo[:23], al[:23])
            d.reload(b, seqs[23:])          # at once: no wait of the caller's in between
            d.run(b, x)
            d.add(t, b, lo[23:], al[23:])
            same(d.fetch(t, nl), R.planted_typing(p, x, "shuffled"), ("reloaded", x))
            d.reload(b, seqs[:23])
        # a batch destroyed right behind its add, and the caller's label arrays overwritten right behind it
        d.reset(t)
        d.run(b, thr)
        d.add(t, b, lo[:23], al[:23])
        b3 = d.batch(seqs[23:])
        d.run(b3, thr)
        my_lo, my_al = np.ascontiguousarray(lo[23:]), np.ascontiguousarray(al[23:])
        assert d.L.bigsi_hip_typing_add_batch(t, b3, ptr(my_lo), ptr(my_al), my_lo.size) == 0
        my_lo[:] = 0
        my_al[:] = 0
        d.free(b3)
        same(d.fetch(t, nl), R.planted_typing(p, thr, "shuffled"), "destroy behind add")
    finally:
        d.destroy(t)
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- streaming
STREAM_LOCI = [0, 1, 1, 2, 0, 0, 0, 1, 2, 1, R.NONE, 2]          # locus 0's records lie in all three chunks; the short query is a record of locus 1
STREAM_ALLELES = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]


def test_stream_over_three_chunks():
    lengths = T.stream_lengths()
    p = T.planted(200, len(lengths), seed=12, lengths=lengths)
    assert T.plan_tally_chunks([len(s) for s in p.seqs], T.K, 4, 4) == [0, 5, 6, 12] and p.us[5] > (1 << 19)
    lo, al = np.array(STREAM_LOCI, np.uint32), np.array(STREAM_ALLELES, np.uint32)
    assert {int(np.searchsorted([5, 6], i, side="right")) for i in np.flatnonzero(lo == 0)} == {0, 1, 2}
    order = np.arange(12)
    d = Dev.planted(p)
    t = d.create(3)
    try:
        for x in (1.0, p.edge_threshold()[0]):
            want = R.typing_of(p.us, p.counts, R.hits_of(p, x), order, lo, al, 3)
            assert want["records"].tolist() == [4, 3, 3] and want["best"].any() and (want["hits"] > 1).any()
            d.reset(t)
            d.stream(t, p.seqs, x, lo, al)
            got = d.fetch(t, 3)
            same(got, want, ("stream", x))
            d.reset(t)
            d.stream(t, p.seqs, x, lo, al)
            assert equal(d.fetch(t, 3), got)                               # twice: bit-identical
            # the one-batch answer
            b = d.batch(p.seqs)
            d.run(b, x, SKIP_COMPACT if x == 1.0 else SKIP_COMPACT | SPARSE_COUNTS)
            d.reset(t)
            d.add(t, b, lo, al)
            assert equal(d.fetch(t, 3), got), ("one batch", x)
            d.free(b)
        # a call of nothing but short sequences adds nothing
        d.reset(t)
        d.stream(t, ["ACGT", "", "TTTTTTTT"], 1.0, [0, 1, 2], [0, 1, 2])
        zero = d.fetch(t, 3)
        assert not any(zero[k].any() for k in zero)
    finally:
        d.destroy(t)
        d.close()


# --------------------------------------------------------------------------------------------- refusals and handles
def test_refusals():
    p = R.width_case(65)
    order, lo, al, nl = R.layout("grouped", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    d = Dev.planted(p)
    L = d.L
    b = d.batch(seqs)
    t = d.create(nl)
    blob, off = d.lib.pack_seqs(seqs)
    out = Out(nl, 65)
    tail = (ptr(out.loci), ptr(out.samples), 65, ptr(out.records))
    slot = C.c_void_p()
    n = len(seqs)
    try:
        # NULL arguments
        for rc in (L.bigsi_hip_typing_create(None, nl, None, C.byref(slot)), L.bigsi_hip_typing_create(d.ix, nl, None, None), L.bigsi_hip_typing_reset(None),
                   L.bigsi_hip_typing_add_batch(None, b, ptr(lo), ptr(al), n), L.bigsi_hip_typing_add_batch(t, None, ptr(lo), ptr(al), n),
                   L.bigsi_hip_typing_add_batch(t, b, None, ptr(al), n), L.bigsi_hip_typing_add_batch(t, b, ptr(lo), None, n),
                   L.bigsi_hip_typing_add_stream(None, blob, ptr(off), n, T.K, 1.0, ptr(lo), ptr(al)), L.bigsi_hip_typing_add_stream(t, blob, None, n, T.K, 1.0, ptr(lo), ptr(al)),
                   L.bigsi_hip_typing_add_stream(t, blob, ptr(off), n, T.K, 1.0, None, ptr(al)), L.bigsi_hip_typing_add_stream(t, blob, ptr(off), n, T.K, 1.0, ptr(lo), None),
                   L.bigsi_hip_typing_add_stream(t, None, ptr(off), n, T.K, 1.0, ptr(lo), ptr(al)),
                   L.bigsi_hip_typing_fetch(None, ptr(out.best), ptr(out.hits), nl * 65, *tail), L.bigsi_hip_typing_fetch(t, ptr(out.best), ptr(out.hits), nl * 65, None, *tail[1:]),
                   L.bigsi_hip_typing_fetch(t, ptr(out.best), ptr(out.hits), nl * 65, tail[0], None, 65, tail[3]),
                   L.bigsi_hip_typing_fetch(t, ptr(out.best), ptr(out.hits), nl * 65, *tail[:3], None)):
            assert rc == ERR_INVALID and d.raw.err()
        assert out.untouched() and L.bigsi_hip_typing_destroy(None) == 0
        # n_loci; cells above the design limit name the numbers
        for bad in (0, (1 << 20) + 1):
            rc, h = d.create_rc(bad)
            assert rc == ERR_INVALID and not h.value and b"BIGSI_TYPING_MAX_LOCI" in d.raw.err()
        wide = Raw(64, 775, h=3)                                             # 13 result words: 2^20 loci would take 9.75 GiB of cells
        assert L.bigsi_hip_typing_create(wide.ix, 1 << 20, None, C.byref(slot)) == ERR_NOMEM and not slot.value
        assert b"BIGSI_TYPING_CELL_BYTES" in d.raw.err() and b"1048576 x 13 x 64 x 12" in d.raw.err()
        wide.close()
        # what a stream's arguments are refused for, and the labels: a bad value names its record and nothing is added
        d.run(b, 1.0)
        down = off.copy()
        down[2] = down[1] - 1
        for m, k, x, o in ((0, T.K, 1.0, off), (n, 0, 1.0, off), (n, T.K, 1.5, off), (n, T.K, float("nan"), off), (n, T.K, 1.0, down)):
            assert L.bigsi_hip_typing_add_stream(t, blob, ptr(o), m, k, x, ptr(lo), ptr(al)) == ERR_INVALID
        wrong = lo.copy()
        wrong[7] = nl
        assert d.add_rc(t, b, wrong, al) == ERR_INVALID and b"locus_of[7]" in d.raw.err()
        assert d.stream_rc(t, seqs, 1.0, wrong, al) == ERR_INVALID and b"locus_of[7]" in d.raw.err()
        wrong[7] = 0xFFFFFFFE
        assert d.add_rc(t, b, wrong, al) == ERR_INVALID and b"locus_of[7]" in d.raw.err()
        wrong = al.copy()
        wrong[9] = 0xFFFFFFFF
        assert d.add_rc(t, b, lo, wrong) == ERR_INVALID and b"allele_of[9]" in d.raw.err() and b"BIGSI_TYPING_MAX_ALLELE" in d.raw.err()
        assert d.stream_rc(t, seqs, 1.0, lo, wrong) == ERR_INVALID and b"allele_of[9]" in d.raw.err()
        for n_entries in (n - 1, n + 1):
            assert d.add_rc(t, b, np.append(lo, 0), np.append(al, 0), n_entries) == ERR_INVALID and b"entries" in d.raw.err()
        zero = d.fetch(t, nl)
        assert not any(zero[k].any() for k in zero)
        # capacity: nothing written
        d.add(t, b, lo, al)
        for kw in (dict(cell_cap=nl * 65 - 1), dict(sample_cap=64)):
            rc, o = d.fetch_rc(t, nl, **kw)
            assert rc == ERR_CAPACITY and o.untouched()
        rc, o = d.fetch_rc(t, nl, cells=False, cell_cap=0)
        assert rc == 0 and not o.untouched()                                # no cells asked for: no cell capacity needed
        # a batch that has not run; one whose run built hit lists; a batch of another index
        fresh = d.batch(seqs)
        assert d.add_rc(t, fresh, lo, al) == ERR_STATE and b"not completed" in d.raw.err()
        d.free(fresh)
        for thr in (1.0, 0.5):
            d.run(b, thr, flags=0)
            assert d.add_rc(t, b, lo, al) == ERR_STATE and b"a typing takes a run made with BIGSI_RUN_SKIP_COMPACT" in d.raw.err()
        other = Dev.planted(p)
        ob = other.batch(seqs)
        other.run(ob, 1.0)
        assert d.add_rc(t, ob, lo, al) == ERR_STATE and b"another index" in d.raw.err()
        other.free(ob)
        other.close()
        # a result limit, caller-owned bit vectors, a result width
        d.run(b, 1.0)
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 5, None, 0))
        assert d.add_rc(t, b, lo, al) == ERR_STATE and b"limit" in d.raw.err() and b"a typing ranks every hit" in d.raw.err()
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 0, None, 0))
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, C.c_void_p(d.info(b).d_bitmaps)))
        assert d.add_rc(t, b, lo, al) == ERR_STATE
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, None))
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 64))
        assert d.add_rc(t, b, lo, al) == ERR_STATE
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 0))
        # the index changed since create: num_hashes, num_cols -- every call but destroy
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, 2))
        assert d.add_rc(t, b, lo, al) == ERR_STATE and b"bigsi_hip_typing_create" in d.raw.err()
        assert L.bigsi_hip_typing_reset(t) == ERR_STATE and d.stream_rc(t, seqs, 1.0, lo, al) == ERR_STATE
        rc, o = d.fetch_rc(t, nl)
        assert rc == ERR_STATE and o.untouched()
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, T.H))
        d.lib.check(L.bigsi_hip_set_num_cols(d.ix, 64))
        rc, o = d.fetch_rc(t, nl)
        assert rc == ERR_STATE and o.untouched() and d.add_rc(t, b, lo, al) == ERR_STATE
        d.lib.check(L.bigsi_hip_set_num_cols(d.ix, 65))
        # ... and the accumulator is fine: it holds the one add from above
        same(d.fetch(t, nl), R.planted_typing(p, 1.0, "grouped"), "after the refusals")
        # an index without columns
        empty = Raw(64, 0, cap=8, h=3)
        assert L.bigsi_hip_typing_create(empty.ix, 1, None, C.byref(slot)) == ERR_STATE and not slot.value
        empty.close()
    finally:
        d.destroy(t)
        d.free(b)
        d.close()


def test_hits_against_the_hit_lists_of_search_batch():
    """hits[l][s] is the number of records of locus l whose bigsi_hip_search_batch hit list holds s, and best's score the largest
    count / unique among them -- the library's own hit lists, a route that shares no kernel with the consumer"""
    p = R.width_case(129)
    order, lo, al, nl = R.layout("interleaved", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    d = Dev.planted(p)
    t = d.create(nl)
    try:
        for thr in (1.0, 0.4):
            blob, off = d.lib.pack_seqs(seqs)
            n = len(seqs)
            nu, hoff = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
            col, cnt = np.zeros(n * 129, np.uint32), np.zeros(n * 129, np.uint32)
            d.lib.check(d.L.bigsi_hip_search_batch(d.ix, blob, ptr(off), n, T.K, thr, 0, None, ptr(nu), None, ptr(hoff), ptr(col), ptr(cnt), col.size))
            hits, score = np.zeros((nl, 129), np.uint32), np.zeros((nl, 129), np.uint64)
            assert (nu == 0).sum() == 1                                      # the query shorter than k: a record without k-mers counts nowhere
            for i in np.flatnonzero(nu):
                for j in range(int(hoff[i]), int(hoff[i + 1])):
                    hits[lo[i], col[j]] += 1
                    score[lo[i], col[j]] = max(int(score[lo[i], col[j]]), int(cnt[j]) * R.EXACT // int(nu[i]))
            assert hits.any() and (hits > 1).any()
            d.reset(t)
            d.stream(t, seqs, thr, lo, al)
            got = d.fetch(t, nl)
            assert np.array_equal(got["hits"], hits) and np.array_equal(got["best"] >> np.uint64(32), score), thr
    finally:
        d.destroy(t)
        d.close()


def test_view_handle():
    p = R.width_case(129)
    order, lo, al, nl = R.layout("grouped", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    columns = R.column_mask(p)[0]
    d = Dev.planted(p)
    view = C.c_void_p()
    d.lib.check(d.L.bigsi_hip_open_view(d.ix, C.byref(view)))
    b = d.batch(seqs, handle=view)
    t = d.create(nl, columns, handle=view)
    try:
        for x in (1.0, 0.4):
            d.reset(t)
            d.run(b, x)
            d.add(t, b, lo, al)
            same(d.fetch(t, nl), R.planted_typing(p, x, "grouped", masked=True), ("view, batch", x))
            d.reset(t)
            d.stream(t, seqs, x, lo, al)
            same(d.fetch(t, nl), R.planted_typing(p, x, "grouped", masked=True), ("view, stream", x))
    finally:
        d.destroy(t)
        d.free(b)
        d.lib.check(d.L.bigsi_hip_close(view))
        d.close()


# --------------------------------------------------------------------------------------------- end to end
def test_type_samples_and_command_line(tmp_path, capsys):
    """BIGSI.type_samples and `typing` on a small built index: a three-locus scheme of three alleles each, samples that hold known
    alleles (one of them only 45 of an allele's 60 bases, one deleted) and a profiles table"""
    import bigsi_amd
    from bigsi_amd import locus_typing as lt
    from bigsi_amd.__main__ import main
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(77)
    k = 11
    loci = ["adk", "fumC", "gyrB"]
    allele = {(l, a): "".join(rng.choice(list("ACGT"), size=60)) for l in loci for a in (1, 2, 3)}
    scheme = "".join(">%s_%d\n%s\n" % (l, a, allele[(l, a)]) for a in (1, 2, 3) for l in loci)          # interleaved in the file: parse_scheme groups
    holds = {"s0": [("adk", 1), ("fumC", 1), ("gyrB", 1)], "s1": [("adk", 2), ("fumC", 1), ("gyrB", 3)], "s2": [("adk", 2), ("fumC", 2), ("gyrB", 2)],
             "s3": [("adk", 1), ("gyrB", 1)], "gone": [("adk", 3), ("fumC", 3), ("gyrB", 3)]}
    seqs = {name: [allele[x] for x in xs] for name, xs in holds.items()}
    seqs["s3"].append(allele[("fumC", 3)][:45])                                                      # 35 of fumC_3's 50 k-mers
    profiles = "ST\tadk\tfumC\tgyrB\tclonal_complex\n1\t1\t1\t1\tCC1\n2\t2\t1\t3\tCC1\n"
    cfg = {"storage-engine": "hip-hbm", "storage-config": {"name": "typing%d" % next(_counter), "filename": str(tmp_path / "index.hbm")}, "k": k, "m": 100003, "h": 3}
    blooms = [bigsi_amd.BIGSI.bloom(cfg, [km for s in ss for km in seq_to_kmers(s, k)]) for ss in seqs.values()]
    b = bigsi_amd.BIGSI.build(cfg, blooms, list(seqs.keys()))
    try:
        b.delete_sample("gone")
        live = ["s0", "s1", "s2", "s3"]
        res = b.type_samples(scheme, profiles=profiles)
        assert [x["name"] for x in res["loci"]] == loci and [s["sample_name"] for s in res["samples"]] == live
        assert [s["ST"] for s in res["samples"]] == ["1", "2", "novel", "-"]
        for s in res["samples"]:
            want = {l: str(a) for l, a in holds[s["sample_name"]]}
            assert {l: c["allele"] for l, c in s["calls"].items()} == want and all(c["exact"] and c["fraction"] == 1.0 and c["n_hits"] == 1 for c in s["calls"].values())
            assert s["called"] == s["exact"] == len(want)
        assert res["loci"] == [{"name": "adk", "records": 3, "called": 4, "exact": 4, "multiple": 0}, {"name": "fumC", "records": 3, "called": 3, "exact": 3, "multiple": 0},
                               {"name": "gyrB", "records": 3, "called": 4, "exact": 4, "multiple": 0}]
        # below threshold 1 the partial allele is called, with its fraction, and still gives no sequence type
        low = b.type_samples(scheme, threshold=0.4, profiles=profiles)
        call = low["samples"][3]["calls"]["fumC"]
        assert call["allele"] == "3" and not call["exact"] and call["fraction"] == (35 * 0xFFFFFFFF // 50) / 0xFFFFFFFF and low["samples"][3]["ST"] == "-"
        assert [s["ST"] for s in low["samples"]] == ["1", "2", "novel", "-"] and low["loci"][1]["called"] == 4 and low["loci"][1]["exact"] == 3
        # a cell budget that forces three slices: five columns are one word, 768 bytes per locus
        _, _, alleles, records, locus_of, allele_of = lt.parse_scheme(scheme)
        assert locus_of.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and allele_of.tolist() == [0, 3, 6, 1, 4, 7, 2, 5, 8] and len(lt.slices(locus_of, 3, 5, 768)) == 3
        assert b.type_samples(scheme, profiles=profiles, cell_bytes=768) == res
        whole, sliced = b.typing_arrays(records, locus_of, 3, allele_of=allele_of), b.typing_arrays(records, locus_of, 3, cell_bytes=768, allele_of=allele_of)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, sliced)) and not whole[0][:, 4].any()          # the deleted sample's cells are zero
        summary = b.type_samples(scheme, summary_only=True)
        assert summary["loci"] == res["loci"] and [dict(s, calls=None, ST=None) for s in summary["samples"]] == [dict(s, calls=None, ST=None) for s in res["samples"]]
        assert b.typing_arrays(records, locus_of, 3, cells=False)[:2] == (None, None)
        # the command line
        b.storage.sync()
        cf, fa, pf = tmp_path / "config.yaml", tmp_path / "scheme.fa", tmp_path / "profiles.tsv"
        cf.write_text(yaml.safe_dump(cfg))
        fa.write_text(scheme)
        pf.write_text(profiles)
        capsys.readouterr()
        argv = ["typing", str(fa), "--profiles", str(pf), "--config", str(cf)]
        assert main(argv) == 0
        text = capsys.readouterr().out
        assert text == lt.to_tsv(res) + "\n"
        assert text.rstrip("\n").split("\n") == ["sample\tST\tadk\tfumC\tgyrB", "s0\t1\t1\t1\t1", "s1\t2\t2\t1\t3", "s2\tnovel\t2\t2\t2", "s3\t-\t1\t-\t1"]
        assert main(argv + ["--format", "json"]) == 0
        assert json.loads(capsys.readouterr().out) == res
        assert main(argv + ["-t", "0.4"]) == 0
        assert capsys.readouterr().out.rstrip("\n").split("\n")[4] == "s3\t-\t1\t3~0.7000\t1"
        assert main(["typing", str(fa), "--config", str(cf), "--summary-only"]) == 0
        assert capsys.readouterr().out == lt.to_tsv(summary, True) + "\n"
        assert main(["typing", str(fa), "--config", str(cf), "--summary-only", "--format", "json"]) == 0
        assert json.loads(capsys.readouterr().out) == summary
    finally:
        b.delete()
