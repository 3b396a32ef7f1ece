"""K-mer prevalence on the device: bigsi_hip_kmer_prevalence / bigsi_hip_batch_kmer_prevalence straight on the C ABI, bit-exact against
numpy on a seeded matrix written with bigsi_hip_set_rows (row ids from the oracle's hashing, junk bits behind num_cols in every row,
sentinels behind `capacity`), then BIGSI.kmer_prevalence / kmer_prevalence_many and the `prevalence` command on an index built from
sequences.  Read-only handles: a view handle is covered; an ipc handle needs a second process that owns the index and is left out."""
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

from conftest import ROOT, load_golden
from raw_index import ptr, rand_seq
from oracle import coracle

pytestmark = pytest.mark.gpu
_counter = itertools.count()
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
SENTINEL = 0xDEADBEEF
K = 31
POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint32)


def pack(seqs):
    data = [s.encode("ascii") for s in seqs]
    off = np.zeros(len(data) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in data])
    return b"".join(data), off


def mask_bytes(flags):
    """bool per column -> the row format, every bit of the last byte past the last column SET (the library must ignore it)."""
    by = np.packbits(flags.astype(np.uint8))
    if flags.size % 8:
        by[-1] |= (1 << (8 - flags.size % 8)) - 1
    return np.ascontiguousarray(by)


class Raw(object):
    """One index straight on the C ABI: m rows of n columns, every row written at the full stride with seeded random bytes (three
    quarters of the bits set), so the whole pad behind column n - 1 holds junk."""

    def __init__(self, m, n, h, seed):
        from bigsi_amd import _lib
        self.L, self.lib = _lib.lib(), _lib
        self.m, self.n, self.h = m, n, h
        self.ix = C.c_void_p()
        _lib.check(self.L.bigsi_hip_open(m, n, n, h, 0, C.byref(self.ix)))
        inf = _lib.Info()
        _lib.check(self.L.bigsi_hip_get_info(self.ix, C.byref(inf)))
        rng = np.random.default_rng(seed)
        stride = int(inf.row_stride_bytes)
        self.rows = np.ascontiguousarray(rng.integers(0, 256, (m, stride), dtype=np.uint8) | rng.integers(0, 256, (m, stride), dtype=np.uint8))
        ids = np.arange(m, dtype=np.uint64)
        _lib.check(self.L.bigsi_hip_set_rows(self.ix, ptr(ids), m, ptr(self.rows), stride))
        self.batches = []

    def want(self, seqs, k, universe=None, subset=None):
        """numpy: (pos_offsets, total, in_subset) from the bytes written; universe / subset as bool[n]."""
        rb = (self.n + 7) // 8
        keep = np.packbits(np.ones(self.n, np.uint8) if universe is None else universe.astype(np.uint8))
        tot, sub, off = [], [], [0]
        for s in seqs:
            ids = coracle.seq_rows(s, k, self.h, self.m)
            if len(ids):
                a = np.bitwise_and.reduce(self.rows[ids.astype(np.int64)][:, :, :rb], axis=1) & keep
                tot.append(POP[a].sum(axis=1, dtype=np.uint32))
                if subset is not None:
                    sub.append(POP[a & np.packbits(subset.astype(np.uint8))].sum(axis=1, dtype=np.uint32))
            off.append(off[-1] + len(ids))
        cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.uint32)      # noqa: E731
        return np.asarray(off, np.uint64), cat(tot), (cat(sub) if subset is not None else None)

    def one_shot(self, seqs, k, universe=None, subset=None, capacity=None, want_sub=None, total_null=False, handle=None):
        blob, off = pack(seqs)
        need = sum(max(len(s) - k + 1, 0) for s in seqs)
        pos = np.full(len(seqs) + 1, SENTINEL, np.uint64)
        tot = np.full(need + 3, SENTINEL, np.uint32)
        sub = np.full(need + 3, SENTINEL, np.uint32) if (subset is not None if want_sub is None else want_sub) else None
        rc = self.L.bigsi_hip_kmer_prevalence(handle or self.ix, blob, ptr(off), len(seqs), k, None if universe is None else ptr(mask_bytes(universe)),
                                              None if subset is None else ptr(mask_bytes(subset)), ptr(pos), None if total_null else ptr(tot), ptr(sub),
                                              need if capacity is None else capacity)
        return rc, pos, tot, sub

    def batch(self, seqs, k):
        blob, off = pack(seqs)
        b = C.c_void_p()
        self.lib.check(self.L.bigsi_hip_batch_create(self.ix, blob, ptr(off), len(seqs), k, C.byref(b)))
        self.batches.append(b)
        return b

    def batch_prevalence(self, b, need, universe=None, subset=None, capacity=None):
        tot = np.full(need + 3, SENTINEL, np.uint32)
        sub = np.full(need + 3, SENTINEL, np.uint32) if subset is not None else None
        rc = self.L.bigsi_hip_batch_kmer_prevalence(b, None if universe is None else ptr(mask_bytes(universe)), None if subset is None else ptr(mask_bytes(subset)),
                                                    ptr(tot), ptr(sub), need if capacity is None else capacity)
        return rc, tot, sub

    def close(self):
        for b in self.batches:
            self.lib.check(self.L.bigsi_hip_batch_destroy(b))
        self.lib.check(self.L.bigsi_hip_close(self.ix))


def check_equal(ix, got, want):
    rc, pos, tot, sub = got
    assert rc == 0, ix.L.bigsi_hip_last_error()
    n = int(want[0][-1])
    assert np.array_equal(pos, want[0])
    assert np.array_equal(tot[:n], want[1]) and (tot[n:] == SENTINEL).all()
    if want[2] is not None:
        assert np.array_equal(sub[:n], want[2]) and (sub[n:] == SENTINEL).all()


def slot_shapes(rng):
    """40 bp (few k-mers: sliced), sequences shorter than k and of exactly k between others, 1 kbp with a 200 bp repeat."""
    a = rand_seq(rng, 800)
    return [rand_seq(rng, 40), rand_seq(rng, K - 1), rand_seq(rng, K), "", a + a[100:300], rand_seq(rng, 64)]


WIDTHS = [1, 63, 64, 65, 8191, 8192, 8193, 3 * 8192 + 70]


@pytest.mark.parametrize("n,h", list(zip(WIDTHS, itertools.cycle([3, 4, 1, 7, 9]))) + [(8193, 1), (3 * 8192 + 70, 9), (3 * 8192 + 70, 7), (8193, 4), (3 * 8192 + 70, 3), (8193, 2), (3 * 8192 + 70, 5), (65, 6)])
def test_widths_hashes_slots_and_masks(n, h):
    """Every width class (the 64-column word, the 16-byte lane, the 1 KiB segment and its multiples) with every kernel instance:
    h = 1 ... 7 are instances of their own, 9 the run-time route with a last group of one row.  These shapes have few k-mers, so
    a slice is one segment and only the predicated last step of a slice runs; test_whole_steps_of_a_slice covers the other loop."""
    rng = np.random.default_rng(1000 * h + n)
    ix = Raw(1009, n, h, seed=n + h)
    try:
        seqs = slot_shapes(rng)
        universe = rng.random(n) < 0.7
        inside = universe & (rng.random(n) < 0.5)
        outside = rng.random(n) < 0.5
        for uni, sub in ((None, None), (universe, None), (None, inside), (universe, inside), (universe, outside), (np.zeros(n, bool), outside)):
            check_equal(ix, ix.one_shot(seqs, K, uni, sub), ix.want(seqs, K, uni, sub))
        want = ix.want(seqs, K)
        dup = int(want[0][4])
        assert np.array_equal(want[1][dup + 100:dup + 170], want[1][dup + 800:dup + 870])          # the repeat carries the same numbers
        if n >= 63:
            assert want[1].max() > 0
    finally:
        ix.close()


@pytest.mark.parametrize("n_seqs", [48, 120])
def test_many_slots_one_slice(n_seqs):
    """n x 200 bp in one call on 10 007 rows of 8193 columns (one whole segment and a one-word second): the unique k-mers exceed
    the planner's wavefront target (4096), so a k-mer is one slice.  48 sequences are 8160 slots, at most twice the target: a
    wavefront per slot; 120 are 20 400: 4096 wavefronts stride over them, five slots each."""
    rng = np.random.default_rng(n_seqs)
    ix = Raw(10007, 8193, 4, seed=7)
    try:
        seqs = [rand_seq(rng, 200) for _ in range(n_seqs)]
        seqs[17] = seqs[3]          # a sequence twice: two sets of slots, the same numbers
        subset = rng.random(8193) < 0.3
        want = ix.want(seqs, K, None, subset)
        assert int(want[0][-1]) == n_seqs * 170 > 4096 and (n_seqs * 170 > 2 * 4096) == (n_seqs == 120)
        check_equal(ix, ix.one_shot(seqs, K, None, subset), want)
    finally:
        ix.close()


@pytest.fixture(scope="module")
def wide_queries():
    rng = np.random.default_rng(17)
    return [rand_seq(rng, 200) for _ in range(30)], slot_shapes(rng)


@pytest.mark.parametrize("h", [1, 2, 3, 4, 5, 6, 7, 9])
def test_whole_steps_of_a_slice(h, wide_queries):
    """The unpredicated loop over whole steps (ceil(8 / h) segments at a time), which carries every wide index: 17 x 8192 + 70
    columns are 17 whole 1 KiB segments and a two-word 18th.  30 x 200 bp are 5100 unique k-mers, beyond the planner's target: one
    slice of all 18 segments -- h = 1: two steps of 8 and a rest of 2; h = 2: four of 4 and 2; h = 3: five of 3 and 3; h = 4 ... 7:
    eight of 2 and 2; h = 9: 17 whole segments and the ragged one.  The ~880 unique k-mers of slot_shapes are cut into five slices of
    4, 4, 4, 4 and 2 segments: whole steps that start in the middle of a row.  Masks differ from segment to segment, so a mask
    read at another segment's offset shows."""
    n = 17 * 8192 + 70
    many, few = wide_queries
    rng = np.random.default_rng(h)
    ix = Raw(1009, n, h, seed=100 + h)
    try:
        universe = rng.random(n) < 0.7
        subset = rng.random(n) < 0.4
        assert sum(len(s) - K + 1 for s in many) == 30 * 170 > 4096
        for seqs in (many, few):
            check_equal(ix, ix.one_shot(seqs, K), ix.want(seqs, K))
            check_equal(ix, ix.one_shot(seqs, K, universe, subset), ix.want(seqs, K, universe, subset))
        assert ix.want(few, K)[1].max() > 0
    finally:
        ix.close()


def test_batch_call_after_every_kind_of_run():
    """bigsi_hip_batch_kmer_prevalence equals the one-shot call after an exact run, a thresholded run and the one-launch read
    route (61 bp reads on a narrow index); and total == popcount of bigsi_hip_batch_lookup's rows."""
    from bigsi_amd import _lib
    rng = np.random.default_rng(5)
    ix = Raw(1009, 8191, 3, seed=11)
    try:
        a = rand_seq(rng, 300)
        long_seqs = [a + a[50:150], rand_seq(rng, K - 2), rand_seq(rng, 400)]
        reads = [rand_seq(rng, 61) for _ in range(9)] + [rand_seq(rng, 20), rand_seq(rng, K)]
        universe = rng.random(8191) < 0.8
        subset = rng.random(8191) < 0.4
        for seqs, thr, flags, one_launch in ((long_seqs, 1.0, 0, 0), (long_seqs, 0.4, 0, 0), (reads, 1.0, 0, 1), (reads, 0.4, _lib.RUN_SPARSE_COUNTS, 1)):
            want = ix.want(seqs, K, universe, subset)
            need = int(want[0][-1])
            b = ix.batch(seqs, K)
            rc, tot, sub = ix.batch_prevalence(b, need)
            assert rc == ERR_STATE and (tot == SENTINEL).all()          # has not run
            _lib.check(ix.L.bigsi_hip_batch_run(b, C.c_double(thr), flags))
            info = _lib.BatchInfo()
            _lib.check(ix.L.bigsi_hip_batch_get_info(b, C.byref(info)))
            assert info.one_launch == one_launch and info.total_kmers == need
            rc, tot, sub = ix.batch_prevalence(b, need, universe, subset)
            assert rc == 0, ix.L.bigsi_hip_last_error()
            assert np.array_equal(tot[:need], want[1]) and np.array_equal(sub[:need], want[2]) and (tot[need:] == SENTINEL).all() and (sub[need:] == SENTINEL).all()
            check_equal(ix, ix.one_shot(seqs, K, universe, subset), want)
            # errors of the batch call
            rc, tot, _ = ix.batch_prevalence(b, need, capacity=need - 1)
            assert rc == ERR_CAPACITY and (tot == SENTINEL).all()
            assert ix.L.bigsi_hip_batch_kmer_prevalence(b, None, None, None, None, need) == ERR_INVALID
            one = np.zeros(need, np.uint32)
            assert ix.L.bigsi_hip_batch_kmer_prevalence(b, None, None, ptr(one), ptr(one), need) == ERR_INVALID
            assert ix.L.bigsi_hip_batch_kmer_prevalence(b, None, ptr(mask_bytes(subset)), ptr(one), None, need) == ERR_INVALID
        # against the library's other route: the AND rows of the unique k-mers of sequence 0 of the last exact long batch
        b = ix.batch(long_seqs, K)
        _lib.check(ix.L.bigsi_hip_batch_run(b, C.c_double(1.0), 0))
        want = ix.want(long_seqs, K)
        rc, tot, _ = ix.batch_prevalence(b, int(want[0][-1]))
        assert rc == 0
        first, p2u = coracle.unique_kmers(long_seqs[0], K)
        u, rb = len(first), (8191 + 7) // 8
        assert u == 300 < len(p2u) == 370
        fp, rows = np.zeros(u, np.uint32), np.zeros((u, rb), np.uint8)
        _lib.check(ix.L.bigsi_hip_batch_lookup(b, 0, ptr(fp), ptr(rows), u))
        rows[:, -1] &= 0xFE          # 8191 columns: the last bit of the last byte is no column
        assert np.array_equal(fp, first) and np.array_equal(POP[rows].sum(axis=1, dtype=np.uint32), tot[fp])
        assert np.array_equal(tot[:370], POP[rows].sum(axis=1, dtype=np.uint32)[p2u])
    finally:
        ix.close()


def test_errors_of_the_one_shot_call():
    rng = np.random.default_rng(9)
    ix = Raw(1009, 100, 3, seed=3)
    try:
        seqs = [rand_seq(rng, 50), rand_seq(rng, 10), rand_seq(rng, 33)]
        want = ix.want(seqs, K)
        need = int(want[0][-1])
        rc, pos, tot, _ = ix.one_shot(seqs, K, capacity=need - 1)
        assert rc == ERR_CAPACITY and b"needed" in ix.L.bigsi_hip_last_error() and np.array_equal(pos, want[0]) and (tot == SENTINEL).all()
        assert ix.one_shot(seqs, K, total_null=True)[0] == ERR_INVALID
        rc, _, tot, sub = ix.one_shot(seqs, K, want_sub=True)                                   # in_subset without subset
        assert rc == ERR_INVALID and (tot == SENTINEL).all() and (sub == SENTINEL).all()
        assert ix.one_shot(seqs, K, subset=np.ones(100, bool), want_sub=False)[0] == ERR_INVALID          # subset without in_subset
        assert ix.one_shot(seqs, 0)[0] == ERR_INVALID
        blob, off = pack(seqs)
        one = np.zeros(need, np.uint32)
        assert ix.L.bigsi_hip_kmer_prevalence(ix.ix, blob, ptr(off), 3, K, None, None, None, ptr(one), None, need) == ERR_INVALID      # NULL pos_offsets
        assert ix.L.bigsi_hip_kmer_prevalence(ix.ix, blob, ptr(off), 0, K, None, None, ptr(np.zeros(4, np.uint64)), ptr(one), None, need) == ERR_INVALID
        assert ix.L.bigsi_hip_kmer_prevalence(None, blob, ptr(off), 3, K, None, None, ptr(np.zeros(4, np.uint64)), ptr(one), None, need) == ERR_INVALID
        check_equal(ix, ix.one_shot(seqs, K), want)          # the handle is fine afterwards
        # only sequences without k-mers: nothing to sweep
        rc, pos, tot, _ = ix.one_shot(["ACGT", ""], K)
        assert rc == 0 and pos.tolist() == [0, 0, 0] and (tot == SENTINEL).all()
    finally:
        ix.close()


def test_view_handle_gives_the_owners_numbers():
    rng = np.random.default_rng(21)
    ix = Raw(1009, 8193, 3, seed=5)
    view = C.c_void_p()
    ix.lib.check(ix.L.bigsi_hip_open_view(ix.ix, C.byref(view)))
    try:
        seqs = slot_shapes(rng)
        universe, subset = rng.random(8193) < 0.6, rng.random(8193) < 0.5
        want = ix.want(seqs, K, universe, subset)
        check_equal(ix, ix.one_shot(seqs, K, universe, subset, handle=view), want)
        check_equal(ix, ix.one_shot(seqs, K, universe, subset), want)
    finally:
        ix.lib.check(ix.L.bigsi_hip_close(view))
        ix.close()


# --------------------------------------------------------------------------------------------- BIGSI level
KB, M, H = 11, 100003, 3          # (a filter wide enough that none of the planted counts below meets a Bloom false positive)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """Six samples; `probe` is planted in s1, s3 and s4 and nowhere else.  The expected numbers come from the samples' own Bloom
    filters (BIGSI.bloom) and the oracle's row ids, so a Bloom false positive counts on both sides."""
    from bigsi_amd import BIGSI
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(31)
    probe = rand_seq(rng, 40)
    seqs = {"s0": rand_seq(rng, 200), "s1": rand_seq(rng, 100) + probe + rand_seq(rng, 60), "s2": rand_seq(rng, 300), "s3": probe + rand_seq(rng, 150),
            "s4": rand_seq(rng, 90) + probe, "s5": rand_seq(rng, 250)}
    d = tmp_path_factory.mktemp("prevalence")
    c = {"storage-engine": "hip-hbm", "k": KB, "m": M, "h": H, "storage-config": {"name": "prevalence%d" % next(_counter), "filename": str(d / "index.hbm")}}
    b = BIGSI.build_from_sequences(c, {n: [s] for n, s in seqs.items()})
    filters = [np.unpackbits(np.frombuffer(BIGSI.bloom(c, list(seq_to_kmers(s, KB))).tobytes(), dtype=np.uint8))[:M].astype(bool) for s in seqs.values()]
    yield {"b": b, "cfg": c, "dir": d, "names": list(seqs), "filters": filters, "seqs": seqs, "probe": probe}
    b.delete()


def want_counts(filters, seq, colours):
    return [sum(1 for c in colours if all(filters[c][r] for r in rows)) for rows in coracle.seq_rows(seq, KB, H, M).astype(np.int64)]


def test_bigsi_kmer_prevalence(small):
    b, filters, probe, names = small["b"], small["filters"], small["probe"], small["names"]
    everyone = list(range(6))
    query = probe + "ACGTACGTACGTTTGACCA" + probe[:15]
    r = b.kmer_prevalence(query)
    assert list(r) == ["num_kmers", "num_unique", "num_samples", "subset_size", "samples_with_kmer", "subset_with_kmer"]
    n = len(query) - KB + 1
    assert r["num_kmers"] == n and r["num_unique"] == len({query[i:i + KB] for i in range(n)}) < n and r["num_samples"] == 6
    assert r["subset_size"] is None and r["subset_with_kmer"] is None
    assert r["samples_with_kmer"] == want_counts(filters, query, everyone)
    assert r["samples_with_kmer"][:30] == [3] * 30 and min(r["samples_with_kmer"]) == 0          # the planted k-mers: exactly three samples
    # a subset splits it
    r = b.kmer_prevalence(query, samples=["s3", "s0", "s2"])
    assert r["subset_size"] == 3 and r["samples_with_kmer"][:30] == [3] * 30 and r["subset_with_kmer"][:30] == [1] * 30
    assert r["subset_with_kmer"] == want_counts(filters, query, [0, 2, 3])
    # many: one device call, records in input order, a sequence shorter than k among them
    many = b.kmer_prevalence_many([query, "ACGT", small["seqs"]["s2"][:80]], samples=["s1", "s4"])
    assert many[0]["subset_with_kmer"][:30] == [2] * 30 and many[1] == {"num_kmers": 0, "num_unique": 0, "num_samples": 6, "subset_size": 2, "samples_with_kmer": [], "subset_with_kmer": []}
    assert many[2]["samples_with_kmer"] == want_counts(filters, small["seqs"]["s2"][:80], everyone) and min(many[2]["samples_with_kmer"]) >= 1
    assert b.kmer_prevalence_many([]) == []
    for bad in ("nobody", "s9"):
        with pytest.raises(ValueError) as e:
            b.kmer_prevalence(query, samples=["s1", bad])
        assert bad in str(e.value)
    with pytest.raises(ValueError):
        b.kmer_prevalence("ACGTé" * 5)
    # a deleted sample leaves the universe, and cannot be named
    b.delete_sample("s3")
    r = b.kmer_prevalence(query)
    assert r["num_samples"] == 5 and r["samples_with_kmer"][:30] == [2] * 30 and r["samples_with_kmer"] == want_counts(filters, query, [0, 1, 2, 4, 5])
    with pytest.raises(ValueError) as e:
        b.kmer_prevalence(query, samples=["s3"])
    assert "s3" in str(e.value)
    assert b.kmer_prevalence(query, samples=["s1", "s2"])["subset_with_kmer"][:30] == [1] * 30
    small["names"] = [nm for nm in names if nm != "s3"]


def test_matrix_wider_than_the_metadata():
    """Columns the metadata has no record of (written ahead of their names) are in no universe: masks are as wide as the matrix,
    the counts as if those columns were not there."""
    from bigsi_amd import BIGSI
    rng = np.random.default_rng(77)
    probe = rand_seq(rng, 30)
    c = {"storage-engine": "hip-hbm", "k": KB, "m": M, "h": H, "storage-config": {"name": "prevalence-wide-%d" % next(_counter)}}
    b = BIGSI.build_from_sequences(c, {"a": [probe + rand_seq(rng, 50)], "b": [rand_seq(rng, 80)], "c": [rand_seq(rng, 20) + probe]})
    try:
        assert b.kmer_prevalence(probe)["samples_with_kmer"] == [2] * 20
        b.bitmatrix.set_num_cols(11)
        b.storage.insert_kmers(9, [probe], KB)          # a column of the matrix that no sample record names
        r = b.kmer_prevalence(probe, samples=["c", "b"])
        assert r["num_samples"] == 3 and r["subset_size"] == 2 and r["samples_with_kmer"] == [2] * 20 and r["subset_with_kmer"] == [1] * 20
        pos, total, _ = b.storage.kmer_prevalence([probe], KB)          # (without a universe the column counts)
        assert total.tolist() == [3] * 20
    finally:
        b.delete()


def test_cli_prevalence(small, capsys):
    """`python -m bigsi_amd prevalence` in a process of its own on the index's snapshot; the other forms through the same main()."""
    from bigsi_amd.__main__ import main
    b, d, probe = small["b"], small["dir"], small["probe"]
    b.storage.sync()
    cf = d / "config.yaml"
    cf.write_text(yaml.safe_dump(small["cfg"]))
    want = dict({"query": probe}, **b.kmer_prevalence(probe, samples=["s1", "s5"]))
    r = subprocess.run([sys.executable, "-m", "bigsi_amd", "prevalence", probe, "-s", "s1", "-s", "s5", "--config", str(cf)], cwd=str(d), capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == json.dumps([want]) + "\n" and json.loads(r.stdout)[0]["subset_with_kmer"] == [1] * 30
    fa = d / "q.fa"
    fa.write_text(">a\n%s\n>b\nACGT\n>c\n%s\n" % (probe, small["seqs"]["s0"][:50]))
    (d / "names.txt").write_text("s1\ns5\n")
    capsys.readouterr()
    assert main(["prevalence", "--fasta", str(fa), "--samples-file", str(d / "names.txt"), "--format", "csv", "--config", str(cf)]) == 0
    rows = list(csv.reader(io.StringIO(capsys.readouterr().out)))
    recs = b.kmer_prevalence_many([probe, "ACGT", small["seqs"]["s0"][:50]], samples=["s1", "s5"])
    assert rows[0] == ["record", "pos", "kmer", "samples", "in_subset"] and len(rows) == 1 + 30 + 0 + 40
    assert rows[1] == ["0", "0", probe[:KB], str(recs[0]["samples_with_kmer"][0]), "1"]
    assert [int(x[3]) for x in rows[31:]] == recs[2]["samples_with_kmer"] and [int(x[4]) for x in rows[31:]] == recs[2]["subset_with_kmer"] and rows[31][0] == "2"
    assert main(["prevalence", probe, "--format", "csv", "--config", str(cf)]) == 0
    rows = list(csv.reader(io.StringIO(capsys.readouterr().out)))
    assert len(rows) == 31 and all(x[4] == "" for x in rows[1:])


def test_g2_reference_lookups():
    """The reference's own lookup outputs: a k-mer's count is the number of 1s in its bit string (ATC in both samples, ATT and TTT
    in one each)."""
    from bigsi_amd import BIGSI
    seen = {}
    for g in load_golden("g2_lookup.json"):
        c = {"storage-engine": "hip-hbm", "k": g["k"], "m": g["m"], "h": g["h"], "storage-config": {"name": "prevalence-g2-%d" % next(_counter)}}
        b = BIGSI.build_from_sequences(c, {"s%d" % i: list(s) for i, s in enumerate(g["samples"])})
        try:
            for lk in g["lookups"]:
                kmers = [lk["kmers"]] if isinstance(lk["kmers"], str) else list(lk["kmers"])
                if any(len(km) != g["k"] for km in kmers):
                    continue
                for km, rec in zip(kmers, b.kmer_prevalence_many(kmers)):
                    assert rec["samples_with_kmer"] == [lk["result"][km].count("1")], (km, lk)
                    seen[km] = rec["samples_with_kmer"][0]
        finally:
            b.delete()
    assert seen["ATC"] == 2 and seen["ATT"] == 1 and seen["TTT"] == 1
