"""Panel genotyping on the device (include/bigsi_hip_genotype.h), straight on the C ABI: k_allele_or, k_genotype_variants and
k_genotype_samples against numpy -- oracle.coracle's hashing plus the row bytes (tests/genotype_ref.py over tally_ref's planted
indexes), never a library call -- on indexes written by bigsi_hip_set_rows with junk bits behind num_cols.  Width edges (65, 129 and
775 columns have an odd number of result words: a pad word is there to be misread) under three probe layouts at threshold 1, at a
threshold whose min_kmers sits exactly on a count an edge column holds and at 0, dense and hits-only counters, with and without a
column selection; probe counts around the kernel's tile; variant counts around a workgroup's four; accumulation over calls, reset,
fetch twice and without planes; add / reload / run / add and destroy-behind-add without a host wait; add_stream over three chunks (one
of them a single sequence of 2^20 + 200 positions) and over chunks of nothing but short sequences, twice, bit-identical; every refusal
with preset outputs; a view handle; and BIGSI.genotype_panel / `python -m bigsi_amd genotype` end to end on the golden variant cases
with their deleted sample, against the golden results and BIGSIVariantSearch.genotype_many.  No tolerance anywhere.
tests/test_genotype_host.py asserts, on the CPU, that none of the references is vacuous."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import yaml

import genotype_ref as R
import tally_ref as T
from raw_index import Raw, ptr
from test_genotype_host import GOLDEN, Out, same

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

    def __init__(self, p):
        probe = Raw(T.M, p.n_cols, h=T.H)
        stride = probe.stride
        probe.close()
        self.raw = Raw(T.M, p.n_cols, h=T.H)
        self.L, self.lib, self.ix, self.n_cols = self.raw.L, self.raw.lib, self.raw.ix, p.n_cols
        ids = np.arange(T.M, dtype=np.uint64)
        rows = np.ascontiguousarray(p.junk_rows(stride))
        self.lib.check(self.L.bigsi_hip_set_rows(self.ix, ptr(ids), ids.size, ptr(rows), rows.shape[1]))

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

    def create_rc(self, n_variants, columns=None, handle=None):
        g = C.c_void_p()
        return self.L.bigsi_hip_genotype_create(handle or self.ix, n_variants, ptr(columns), C.byref(g)), g

    def create(self, n_variants, columns=None, handle=None):
        rc, g = self.create_rc(n_variants, columns, handle)
        assert rc == 0 and g.value, self.raw.err()
        return g

    def destroy(self, g):
        self.lib.check(self.L.bigsi_hip_genotype_destroy(g))

    def add_rc(self, g, b, allele_of, n_entries=None):
        allele_of = np.ascontiguousarray(allele_of, np.uint32)
        return self.L.bigsi_hip_genotype_add_batch(g, b, ptr(allele_of), allele_of.size if n_entries is None else n_entries)

    def add(self, g, b, allele_of):
        assert self.add_rc(g, b, allele_of) == 0, self.raw.err()

    def stream_rc(self, g, seqs, thr, allele_of, k=T.K):
        blob, off = self.lib.pack_seqs(seqs)
        allele_of = np.ascontiguousarray(allele_of, np.uint32)
        return self.L.bigsi_hip_genotype_add_stream(g, blob, ptr(off), len(seqs), k, float(thr), ptr(allele_of))

    def stream(self, g, seqs, thr, allele_of):
        assert self.stream_rc(g, seqs, thr, allele_of) == 0, self.raw.err()

    def fetch_rc(self, g, n_variants, planes=True, plane_cap=None, sample_cap=None):
        """(rc, Out) over buffers preset to a pattern, with a guard entry behind each"""
        out = Out(n_variants, self.n_cols)
        rc = self.L.bigsi_hip_genotype_fetch(g, ptr(out.ref) if planes else None, ptr(out.alt) if planes else None, out.nv * out.rb if plane_cap is None else plane_cap,
                                             ptr(out.variants), ptr(out.samples), self.n_cols if sample_cap is None else sample_cap, ptr(out.probes))
        assert out.guards_hold()
        return rc, out

    def fetch(self, g, n_variants, planes=True):
        rc, out = self.fetch_rc(g, n_variants, planes)
        assert rc == 0, self.raw.err()
        if not planes:
            assert out.ref.tobytes() == b"\xab" * out.ref.nbytes and out.alt.tobytes() == b"\xab" * out.alt.nbytes
        return out.got(planes)

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
    d = Dev(p)
    try:
        for name in R.LAYOUTS:
            order, al, nv = R.layout(name, len(p.seqs))
            b = d.batch([p.seqs[q] for q in order])
            accs = {False: d.create(nv), True: d.create(nv, columns)}
            try:
                for thr in R.thresholds(p):
                    for flags in runs_of(thr):
                        d.run(b, thr, flags)
                        assert d.info(b).exact == (1 if thr == 1.0 else 0)
                        for masked, g in accs.items():
                            d.lib.check(d.L.bigsi_hip_genotype_reset(g))
                            d.add(g, b, al)
                            same(d.fetch(g, nv), R.planted_genotype(p, thr, name, masked), ("width", n_cols, name, thr, flags, masked))
            finally:
                for g in accs.values():
                    d.destroy(g)
                d.free(b)
    finally:
        d.close()


@pytest.mark.parametrize("n_seqs", (R.TILE - 1, R.TILE, R.TILE + 1, 2 * R.TILE + 1))
def test_probe_counts_around_the_tile(n_seqs):
    p = T.planted(200, n_seqs, seed=n_seqs)
    order, al, nv = R.layout("interleaved", n_seqs)
    assert n_seqs < 2 * R.TILE or len(set((np.flatnonzero(al == al[32]) // R.TILE).tolist())) == 3          # one allele's probes in three tiles
    d = Dev(p)
    b = d.batch(p.seqs)
    g = d.create(nv)
    try:
        for thr in R.thresholds(p)[:2]:
            d.run(b, thr, SKIP_COMPACT if thr == 1.0 else SKIP_COMPACT | SPARSE_COUNTS)
            d.lib.check(d.L.bigsi_hip_genotype_reset(g))
            d.add(g, b, al)
            want = R.planted_genotype(p, thr, "interleaved")
            assert want["probes"].sum() == n_seqs - 1 and want["ref"].any() and want["alt"].any()          # every probe but the short one counts
            same(d.fetch(g, nv), want, ("probes", n_seqs, thr))
    finally:
        d.destroy(g)
        d.free(b)
        d.close()


@pytest.mark.parametrize("n_variants", (1, 2, 63, 64, 65))
def test_variant_counts(n_variants):
    """nine probes over up to 65 variants: most alleles have no probe, and `used` and `missing` must still be right"""
    p = R.width_case(129)
    order, al, nv = R.layout("interleaved", 9, n_variants)
    d = Dev(p)
    b = d.batch(p.seqs[:9])
    g = d.create(nv)
    try:
        for thr in (1.0, 0.0):
            want = R.planted_genotype(p, thr, "interleaved", sel=9, n_variants=n_variants)
            assert want["variants"].shape == (n_variants, 4) and (want["variants"].sum(axis=1) == 129).all() and want["probes"].sum() == 8
            if n_variants >= 63:
                assert (want["probes"].sum(axis=1) == 0).sum() >= n_variants - 9 and (want["variants"][-1] == [0, 0, 0, 129]).all()
            d.run(b, thr, SKIP_COMPACT if thr == 1.0 else SKIP_COMPACT | SPARSE_COUNTS)
            d.lib.check(d.L.bigsi_hip_genotype_reset(g))
            d.add(g, b, al)
            same(d.fetch(g, nv), want, ("variants", n_variants, thr))
    finally:
        d.destroy(g)
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- accumulation
def test_accumulation_reset_and_fetch():
    p = R.width_case(200)
    order, al, nv = R.layout("grouped", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    want = R.planted_genotype(p, 1.0, "grouped")
    d = Dev(p)
    whole, first, second = d.batch(seqs), d.batch(seqs[:29]), d.batch(seqs[29:])
    g = d.create(nv)
    try:
        for b in (whole, first, second):
            d.run(b, 1.0)
        # two halves in two calls are one whole
        d.add(g, first, al[:29])
        half = d.fetch(g, nv)
        assert not equal(half, want) and half["probes"].sum() < want["probes"].sum()
        d.add(g, second, al[29:])
        both = d.fetch(g, nv)
        same(both, want, "two halves")
        # fetch twice: identical; without planes: the same counts, no plane written
        assert equal(d.fetch(g, nv), both)
        counts_only = d.fetch(g, nv, planes=False)
        assert all(counts_only[k].tobytes() == both[k].tobytes() for k in ("variants", "samples", "probes"))
        # the planes keep accumulating behind a fetch: the same batch again gives the same planes and doubled `used`
        d.add(g, whole, al)
        again = d.fetch(g, nv)
        assert all(again[k].tobytes() == both[k].tobytes() for k in ("ref", "alt", "variants", "samples")) and np.array_equal(again["probes"], 2 * want["probes"])
        # reset zeroes
        d.lib.check(d.L.bigsi_hip_genotype_reset(g))
        zero = d.fetch(g, nv)
        assert not zero["ref"].any() and not zero["alt"].any() and not zero["probes"].any() and not zero["samples"].any()
        assert (zero["variants"] == [0, 0, 0, 200]).all()
        d.add(g, whole, al)
        same(d.fetch(g, nv), want, "after reset")
    finally:
        d.destroy(g)
        for b in (whole, first, second):
            d.free(b)
        d.close()


def test_add_reload_run_add_without_a_wait():
    p = R.width_case(200)
    thr = R.thresholds(p)[1]
    order, al, nv = R.layout("shuffled", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    d = Dev(p)
    b = d.batch(seqs[:23])
    g = d.create(nv)
    try:
        for x in (1.0, thr):
            d.lib.check(d.L.bigsi_hip_genotype_reset(g))
            d.run(b, x)
            d.add(g, b, al[:23])
            d.reload(b, seqs[23:])          # at once: no wait of the caller's in between
            d.run(b, x)
            d.add(g, b, al[23:])
            same(d.fetch(g, nv), R.planted_genotype(p, x, "shuffled"), ("reloaded", x))
            d.reload(b, seqs[:23])
        # a batch destroyed right behind its add, and the caller's allele_of overwritten right behind it
        d.lib.check(d.L.bigsi_hip_genotype_reset(g))
        d.run(b, thr)
        d.add(g, b, al[:23])
        b3 = d.batch(seqs[23:])
        d.run(b3, thr)
        mine = np.ascontiguousarray(al[23:])
        assert d.L.bigsi_hip_genotype_add_batch(g, b3, ptr(mine), mine.size) == 0
        mine[:] = 0
        d.free(b3)
        same(d.fetch(g, nv), R.planted_genotype(p, thr, "shuffled"), "destroy behind add")
    finally:
        d.destroy(g)
        d.free(b)
        d.close()


# --------------------------------------------------------------------------------------------- streaming
STREAM_ALLELES = [0, 2, 3, 4, 1, 0, 0, 1, 5, 2, R.NONE, 4]          # variant 0's ref probes lie in all three chunks; variant 1's only alt probe is the short query


def test_stream_over_three_chunks():
    lengths = T.stream_lengths()
    p = T.planted(200, len(lengths), seed=12, lengths=lengths)
    assert T.plan_tally_chunks([len(s) for s in p.seqs], T.K, 4, 4) == [0, 5, 6, 12] and p.us[5] > (1 << 19)
    al = np.array(STREAM_ALLELES, np.uint32)
    assert {int(np.searchsorted([5, 6], i, side="right")) for i in np.flatnonzero(al == 0)} == {0, 1, 2}
    order = np.arange(12)
    d = Dev(p)
    g = d.create(3)
    try:
        for x in (1.0, p.edge_threshold()[0]):
            want = R.genotype_of(p.us, R.hits_of(p, x), order, al, 3)
            assert want["probes"].tolist() == [[3, 2], [2, 0], [2, 1]] and want["ref"].any() and want["alt"].any()
            for sel in (slice(0, 5), slice(5, 6), slice(6, 12)):          # every chunk has bits of its own to get wrong (the long sequence below threshold 1 only)
                part = R.genotype_of(p.us, R.hits_of(p, x), order[sel], al[sel], 3)
                assert part["ref"].any() or part["alt"].any() or (x == 1.0 and sel.start == 5)
            d.lib.check(d.L.bigsi_hip_genotype_reset(g))
            d.stream(g, p.seqs, x, al)
            got = d.fetch(g, 3)
            same(got, want, ("stream", x))
            d.lib.check(d.L.bigsi_hip_genotype_reset(g))
            d.stream(g, p.seqs, x, al)
            assert equal(d.fetch(g, 3), got)                               # twice: bit-identical
        # add_batch of the whole gives the same
        b = d.batch(p.seqs)
        d.run(b, 1.0)
        d.lib.check(d.L.bigsi_hip_genotype_reset(g))
        d.add(g, b, al)
        want = R.genotype_of(p.us, R.hits_of(p, 1.0), order, al, 3)
        same(d.fetch(g, 3), want, "one batch")
        d.free(b)
        # a call of nothing but short sequences adds nothing; nor does such a chunk between two that do
        d.lib.check(d.L.bigsi_hip_genotype_reset(g))
        d.stream(g, ["ACGT", "", "TTTTTTTT"], 1.0, [0, 1, 2])
        zero = d.fetch(g, 3)
        assert not zero["ref"].any() and not zero["alt"].any() and not zero["probes"].any() and (zero["variants"] == [0, 0, 0, 200]).all()
        filler = ["ACGTACGTAC"] * 4096                                      # a whole chunk (4096 sequences) without a k-mer position
        seqs = filler[:4091] + p.seqs[:5] + filler + p.seqs[6:]
        assert T.plan_tally_chunks([len(s) for s in seqs], T.K, 4, 0) == [0, 4096, 8192, 8198]
        alleles = np.concatenate([np.full(4091, 1, np.uint32), al[:5], np.full(4096, 3, np.uint32), al[6:]])
        d.stream(g, seqs, 1.0, alleles)
        sel = np.r_[0:5, 6:12]
        same(d.fetch(g, 3), R.genotype_of(p.us, R.hits_of(p, 1.0), order[sel], al[sel], 3), "around a chunk of short sequences")
    finally:
        d.destroy(g)
        d.close()


# --------------------------------------------------------------------------------------------- refusals and handles
def test_refusals():
    p = R.width_case(65)
    order, al, nv = R.layout("grouped", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    d = Dev(p)
    L = d.L
    b = d.batch(seqs)
    g = d.create(nv)
    blob, off = d.lib.pack_seqs(seqs)
    out = Out(nv, 65)
    tail = (ptr(out.variants), ptr(out.samples), 65, ptr(out.probes))
    slot = C.c_void_p()
    try:
        # NULL arguments
        for rc in (L.bigsi_hip_genotype_create(None, nv, None, C.byref(slot)), L.bigsi_hip_genotype_create(d.ix, nv, None, None), L.bigsi_hip_genotype_reset(None),
                   L.bigsi_hip_genotype_add_batch(None, b, ptr(al), al.size), L.bigsi_hip_genotype_add_batch(g, None, ptr(al), al.size),
                   L.bigsi_hip_genotype_add_batch(g, b, None, al.size), L.bigsi_hip_genotype_add_stream(None, blob, ptr(off), len(seqs), T.K, 1.0, ptr(al)),
                   L.bigsi_hip_genotype_add_stream(g, blob, None, len(seqs), T.K, 1.0, ptr(al)), L.bigsi_hip_genotype_add_stream(g, blob, ptr(off), len(seqs), T.K, 1.0, None),
                   L.bigsi_hip_genotype_add_stream(g, None, ptr(off), len(seqs), T.K, 1.0, ptr(al)),
                   L.bigsi_hip_genotype_fetch(None, ptr(out.ref), ptr(out.alt), nv * 9, *tail), L.bigsi_hip_genotype_fetch(g, ptr(out.ref), ptr(out.alt), nv * 9, None, *tail[1:]),
                   L.bigsi_hip_genotype_fetch(g, ptr(out.ref), ptr(out.alt), nv * 9, tail[0], None, 65, tail[3]),
                   L.bigsi_hip_genotype_fetch(g, ptr(out.ref), ptr(out.alt), nv * 9, *tail[:3], None)):
            assert rc == ERR_INVALID and d.raw.err()
        assert out.untouched() and L.bigsi_hip_genotype_destroy(None) == 0
        # n_variants
        for bad in (0, (1 << 20) + 1):
            rc, h = d.create_rc(bad)
            assert rc == ERR_INVALID and not h.value and b"BIGSI_GENOTYPE_MAX_VARIANTS" in d.raw.err()
        # what a stream's arguments are refused for, and allele_of: nothing is added
        d.run(b, 1.0)
        down = off.copy()
        down[2] = down[1] - 1
        for n, k, x, o in ((0, T.K, 1.0, off), (len(seqs), 0, 1.0, off), (len(seqs), T.K, 1.5, off), (len(seqs), T.K, float("nan"), off), (len(seqs), T.K, 1.0, down)):
            assert L.bigsi_hip_genotype_add_stream(g, blob, ptr(o), n, k, x, ptr(al)) == ERR_INVALID
        wrong = al.copy()
        wrong[7] = 2 * nv
        assert d.add_rc(g, b, wrong) == ERR_INVALID and b"allele_of[7]" in d.raw.err()
        assert d.stream_rc(g, seqs, 1.0, wrong) == ERR_INVALID and b"allele_of[7]" in d.raw.err()
        wrong[7] = 0xFFFFFFFE
        assert d.add_rc(g, b, wrong) == ERR_INVALID and b"allele_of[7]" in d.raw.err()
        for n_entries in (len(seqs) - 1, len(seqs) + 1):
            assert d.add_rc(g, b, np.append(al, 0), n_entries) == ERR_INVALID and b"entries" in d.raw.err()
        zero = d.fetch(g, nv)
        assert not zero["ref"].any() and not zero["alt"].any() and not zero["probes"].any()
        # capacity: nothing written
        d.add(g, b, al)
        for kw in (dict(plane_cap=nv * 9 - 1), dict(sample_cap=64)):
            rc, o = d.fetch_rc(g, nv, **kw)
            assert rc == ERR_CAPACITY and o.untouched()
        rc, o = d.fetch_rc(g, nv, planes=False, plane_cap=0)
        assert rc == 0 and not o.untouched()                                # no plane asked for: no plane capacity needed
        # a batch that has not run; one whose run built hit lists; a batch of another index
        fresh = d.batch(seqs)
        assert d.add_rc(g, fresh, al) == ERR_STATE and b"not completed" in d.raw.err()
        d.free(fresh)
        for thr in (1.0, 0.5):
            d.run(b, thr, flags=0)
            assert d.add_rc(g, b, al) == ERR_STATE and b"a genotyping takes a run made with BIGSI_RUN_SKIP_COMPACT" in d.raw.err()
        other = Dev(p)
        ob = other.batch(seqs)
        other.run(ob, 1.0)
        assert d.add_rc(g, ob, al) == ERR_STATE and b"another index" in d.raw.err()
        other.free(ob)
        other.close()
        # a result limit, caller-owned bit vectors, a result width
        d.run(b, 1.0)
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 5, None, 0))
        assert d.add_rc(g, b, al) == ERR_STATE and b"limit" in d.raw.err()
        d.lib.check(L.bigsi_hip_batch_set_limit(b, 0, None, 0))
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, C.c_void_p(d.info(b).d_bitmaps)))
        assert d.add_rc(g, b, al) == ERR_STATE
        d.lib.check(L.bigsi_hip_batch_set_outputs(b, None))
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 64))
        assert d.add_rc(g, b, al) == ERR_STATE
        d.lib.check(L.bigsi_hip_batch_set_result_cols(b, 0))
        # the index changed since create: num_hashes, num_cols -- every call but destroy
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, 2))
        assert d.add_rc(g, b, al) == ERR_STATE and b"bigsi_hip_genotype_create" in d.raw.err()
        assert L.bigsi_hip_genotype_reset(g) == ERR_STATE and d.stream_rc(g, seqs, 1.0, al) == ERR_STATE
        rc, o = d.fetch_rc(g, nv)
        assert rc == ERR_STATE and o.untouched()
        d.lib.check(L.bigsi_hip_set_num_hashes(d.ix, T.H))
        d.lib.check(L.bigsi_hip_set_num_cols(d.ix, 64))
        rc, o = d.fetch_rc(g, nv)
        assert rc == ERR_STATE and o.untouched() and d.add_rc(g, b, al) == ERR_STATE
        d.lib.check(L.bigsi_hip_set_num_cols(d.ix, 65))
        # ... and the accumulator is fine: it holds the one add from above
        same(d.fetch(g, nv), R.planted_genotype(p, 1.0, "grouped"), "after the refusals")
        # an index without columns
        empty = Raw(64, 0, cap=8, h=3)
        assert L.bigsi_hip_genotype_create(empty.ix, 1, None, C.byref(slot)) == ERR_STATE and not slot.value
        empty.close()
    finally:
        d.destroy(g)
        d.free(b)
        d.close()


def test_view_handle():
    p = R.width_case(129)
    thr = R.thresholds(p)[1]
    order, al, nv = R.layout("grouped", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    columns = R.column_mask(p)[0]
    d = Dev(p)
    view = C.c_void_p()
    d.lib.check(d.L.bigsi_hip_open_view(d.ix, C.byref(view)))
    b = d.batch(seqs, handle=view)
    g = d.create(nv, columns, handle=view)
    try:
        for x in (1.0, thr):
            d.lib.check(d.L.bigsi_hip_genotype_reset(g))
            d.run(b, x)
            d.add(g, b, al)
            same(d.fetch(g, nv), R.planted_genotype(p, x, "grouped", masked=True), ("view, batch", x))
            d.lib.check(d.L.bigsi_hip_genotype_reset(g))
            d.stream(g, seqs, x, al)
            same(d.fetch(g, nv), R.planted_genotype(p, x, "grouped", masked=True), ("view, stream", x))
    finally:
        d.destroy(g)
        d.free(b)
        d.lib.check(d.L.bigsi_hip_close(view))
        d.close()


# --------------------------------------------------------------------------------------------- end to end
def test_genotype_panel_and_command_line_on_the_golden_cases(tmp_path, capsys):
    """BIGSI.genotype_panel and `genotype` on the index tests/test_variant_search.py builds from g12_variant.json, its deleted sample
    included: per variant the non-missing calls are the golden results, and BIGSIVariantSearch.genotype_many's on the same index."""
    import bigsi_amd
    from bigsi_amd import genotype
    from bigsi_amd.__main__ import main
    from bigsi_amd.utils import seq_to_kmers
    from bigsi_amd.variant_search import BIGSIVariantSearch
    with open(GOLDEN) as f:
        gold = json.load(f)
    cfg = {"storage-engine": "hip-hbm", "storage-config": {"name": "genotype%d" % next(_counter), "filename": str(tmp_path / "index.hbm")},
           "k": gold["k"], "m": gold["m"], "h": gold["h"]}
    blooms = [bigsi_amd.BIGSI.bloom(cfg, [km for s in seqs for km in seq_to_kmers(s, gold["k"])]) for seqs in gold["samples"].values()]
    b = bigsi_amd.BIGSI.build(cfg, blooms, list(gold["samples"].keys()))
    try:
        for name in gold["deleted"]:
            b.delete_sample(name)
        cases = gold["cases"]
        panel = "".join(c["probes_fasta"] for c in cases)
        live = [n for n in gold["samples"] if n not in gold["deleted"]]
        res = b.genotype_panel(panel)
        many = BIGSIVariantSearch(b, "ref.fa").genotype_many([(c["refs"], c["alts"]) for c in cases])
        assert [v["name"] for v in res["variants"]] == [c["query"] for c in cases] and len(cases) == 16
        assert [s["sample_name"] for s in res["samples"]] == live and len(live) == len(gold["samples"]) - 1
        seen = set()
        for v, c, m in zip(res["variants"], cases, many):
            want = {(r["sample_name"], r["genotype"]) for r in c["results"]}
            assert set(v["calls"].items()) == want == {(r["sample_name"], r["genotype"]) for r in m}, c["query"]
            assert v["counts"] == {"0/0": sum(g == "0/0" for _, g in want), "0/1": sum(g == "0/1" for _, g in want), "1/1": sum(g == "1/1" for _, g in want),
                                   "./.": len(live) - len(want)}
            assert (v["ref_probes"], v["alt_probes"]) == (len(c["refs"]), len(c["alts"])) and "uncallable" not in v
            seen |= {g for _, g in want}
        assert seen == {"0/0", "0/1", "1/1"} and any(v["counts"]["./."] for v in res["variants"])
        for s in res["samples"]:
            mine = [v["calls"].get(s["sample_name"]) for v in res["variants"]]
            assert s["carried"] == sum(x in ("0/1", "1/1") for x in mine) and s["called"] == sum(x is not None for x in mine)
        assert any(s["carried"] for s in res["samples"]) and any(s["called"] < 16 for s in res["samples"])
        # a plane budget that forces three slices: seven columns are one word per plane, 16 bytes per variant, and 96 bytes hold 6 of the 16 variants
        names, probes, allele_of = genotype.parse_panel(panel)
        assert len(genotype.slices(allele_of, 16, 1, 96)) == 3
        assert b.genotype_panel(panel, plane_bytes=96) == res
        whole, sliced = b.genotype_arrays(probes, allele_of, 16), b.genotype_arrays(probes, allele_of, 16, plane_bytes=96)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, sliced))
        summary = b.genotype_panel(panel, summary_only=True)
        assert summary["samples"] == res["samples"] and [dict(v, calls=None) for v in summary["variants"]] == [dict(v, calls=None) for v in res["variants"]]
        # a variant whose alt probes are shorter than k cannot be called
        odd = b.genotype_panel(">ref-X1Y\n%s\n>alt-X1Y-0\nACGT\n" % cases[0]["refs"][0])
        assert odd["variants"][0]["uncallable"] is True and odd["variants"][0]["alt_probes"] == 0 and set(odd["variants"][0]["calls"].values()) == {"0/0"}
        # the command line
        b.storage.sync()
        cf, fa = tmp_path / "config.yaml", tmp_path / "panel.fa"
        cf.write_text(yaml.safe_dump(cfg))
        fa.write_text(panel)
        capsys.readouterr()
        argv = ["genotype", str(fa), "--config", str(cf)]
        assert main(argv) == 0
        text = capsys.readouterr().out
        assert text == genotype.to_tsv(res) + "\n"
        lines = text.rstrip("\n").split("\n")
        assert lines[0].split("\t") == ["variant"] + live and len(lines) == 17
        for line, c in zip(lines[1:], cases):
            cells = line.split("\t")
            got = {(n, x) for n, x in zip(live, cells[1:]) if x != "./."}
            assert cells[0] == c["query"] and got == {(r["sample_name"], r["genotype"]) for r in c["results"]}
        assert main(argv + ["--format", "json"]) == 0
        assert json.loads(capsys.readouterr().out) == res
        assert main(argv + ["--summary-only"]) == 0
        assert capsys.readouterr().out == genotype.to_tsv(summary, True) + "\n"
        assert main(argv + ["--summary-only", "--format", "json"]) == 0
        assert json.loads(capsys.readouterr().out) == summary
    finally:
        b.delete()
