"""Sample statistics on the device: bigsi_hip_column_popcounts (k_col_popcount + k_col_popcount_sum) and its group twin against
numpy on the very bit matrix that was written with set_rows -- bit-exact, uint64 -- and BIGSI.sample_stats / similar_samples and the
`stats` / `similar` commands on top of it.  Shapes are the smallest that take every path of the kernel: one and several row blocks
(1920 rows each at these sizes), a flush of the bit-sliced planes inside a block (every 960 rows), ragged widths around the 64-column
word, the 1 KiB segment and the four-segment workgroup, masks whose last byte is ragged."""
import ctypes as C
import csv
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

pytestmark = pytest.mark.gpu
_counter = itertools.count()
ERR_INVALID, ERR_CAPACITY = -1, -5
SENTINEL = 0xDEADBEEF


class Raw(object):
    """One index straight on the C ABI, holding the bit matrix `bits` (uint8[m, n] of 0 / 1) written with bigsi_hip_set_rows."""

    def __init__(self, bits=None, m=None, n=None):
        from bigsi_amd import _lib
        self.L, self.lib = _lib.lib(), _lib
        self.m, self.n = (m, n) if bits is None else bits.shape
        self.ix = C.c_void_p()
        _lib.check(self.L.bigsi_hip_open(self.m, self.n, self.n, 3, 0, C.byref(self.ix)))
        if bits is not None:
            self.write(np.packbits(bits, axis=1))

    def write(self, packed):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        ids = np.arange(self.m, dtype=np.uint64)
        self.lib.check(self.L.bigsi_hip_set_rows(self.ix, ptr(ids), self.m, ptr(packed), packed.shape[1]))

    def counts(self, mask=None, capacity=None, handle=None, size=None):
        """(rc, out): out is `size` entries (default num_cols) preset to a sentinel."""
        out = np.full(self.n if size is None else size, SENTINEL, dtype=np.uint64)
        rc = self.L.bigsi_hip_column_popcounts(handle or self.ix, ptr(mask), ptr(out), out.size if capacity is None else capacity)
        return rc, out

    def close(self):
        self.lib.check(self.L.bigsi_hip_close(self.ix))


def pack_mask(sel, junk=False):
    """Row selector (bool[m]) in the layout get_column writes; junk: every bit of the last byte past row m - 1 set."""
    by = np.packbits(sel.astype(np.uint8))
    if junk and sel.size % 8:
        by[-1] |= (1 << (8 - sel.size % 8)) - 1
    return np.ascontiguousarray(by)


def col_sums(bits, sel=None):
    return (bits if sel is None else bits[sel]).sum(axis=0, dtype=np.uint64)


def test_a_random_unmasked():
    rng = np.random.default_rng(11)
    bits = (rng.random((1009, 200)) < 0.3).astype(np.uint8)
    ix = Raw(bits)
    try:
        rc, got = ix.counts()
        assert rc == 0 and got.dtype == np.uint64 and np.array_equal(got, col_sums(bits))
    finally:
        ix.close()


def test_b_flush_and_counter_width():
    """37 row blocks of 1920 rows, each flushing its planes once on the way (after 960 rows) and once at its end; columns 0 and 129
    count all 70 001 rows -- more than 16 bits and more than any plane capacity; column 64 every other row."""
    rng = np.random.default_rng(12)
    m, n = 70001, 130
    bits = (rng.random((m, n)) < 0.3).astype(np.uint8)
    bits[:, 0] = bits[:, 129] = 1
    bits[:, 64] = (np.arange(m) % 2 == 0)
    ix = Raw(bits)
    try:
        rc, got = ix.counts()
        assert rc == 0 and np.array_equal(got, col_sums(bits))
        assert got[0] == got[129] == 70001 and got[64] == 35001
        # the masked kernel over the same row blocks: a mask of all ones flushes inside a block too, a sparse one does not
        rc, got = ix.counts(pack_mask(np.ones(m, bool), junk=True))
        assert rc == 0 and np.array_equal(got, col_sums(bits))
        sel = rng.random(m) < 0.25
        rc, got = ix.counts(pack_mask(sel))
        assert rc == 0 and np.array_equal(got, col_sums(bits, sel))
    finally:
        ix.close()


# (33 000 columns: five 1 KiB segments, i.e. the second workgroup of a row block)
@pytest.mark.parametrize("n", [1, 8, 63, 64, 65, 127, 128, 129, 1023, 1025, 8191, 8193, 33000])
def test_c_ragged_widths_and_bit_order(n):
    """Column c is set in exactly the rows r < (c * 37) % 258: neighbouring columns differ, so a slip in the in-byte bit order, the word
    order or the segment order shows."""
    m = 257
    want = (np.arange(n, dtype=np.uint64) * 37) % 258
    bits = (np.arange(m)[:, None] < want[None, :]).astype(np.uint8)
    ix = Raw(bits)
    try:
        rc, got = ix.counts()
        assert rc == 0 and np.array_equal(got, want)
    finally:
        ix.close()


def test_d_masks():
    rng = np.random.default_rng(14)
    m, n = 1013, 300
    bits = (rng.random((m, n)) < 0.3).astype(np.uint8)
    sel = rng.random(m) < 0.4
    ix = Raw(bits)
    try:
        rc, got = ix.counts(pack_mask(sel))
        assert rc == 0 and np.array_equal(got, col_sums(bits, sel))
        rc, got = ix.counts(pack_mask(sel, junk=True))                       # bits of the last byte beyond row 1012 change nothing
        assert rc == 0 and np.array_equal(got, col_sums(bits, sel))
        rc, got = ix.counts(pack_mask(np.ones(m, bool)))
        assert rc == 0 and np.array_equal(got, col_sums(bits)) and np.array_equal(got, ix.counts()[1])
        rc, got = ix.counts(pack_mask(np.zeros(m, bool)))
        assert rc == 0 and not got.any()
        one = np.zeros(m, bool)
        one[m - 1] = True                                                    # the last row alone
        rc, got = ix.counts(pack_mask(one, junk=True))
        assert rc == 0 and np.array_equal(got, bits[m - 1].astype(np.uint64))
    finally:
        ix.close()


def test_e_padding_is_never_reported():
    """Rows written at the full stride with all ones: the 28 pad columns of a 100-column index hold bits, and are not counted."""
    from bigsi_amd import _lib
    m, n = 1500, 100
    ix = Raw(m=m, n=n)
    try:
        inf = _lib.Info()
        _lib.check(ix.L.bigsi_hip_get_info(ix.ix, C.byref(inf)))
        assert inf.row_stride_bytes == 128
        ix.write(np.full((m, int(inf.row_stride_bytes)), 0xFF, np.uint8))
        rc, got = ix.counts(size=128)
        assert rc == 0 and (got[:100] == m).all() and (got[100:] == SENTINEL).all()
        rc, got = ix.counts(mask=pack_mask(np.arange(m) < 700), size=128)
        assert rc == 0 and (got[:100] == 700).all() and (got[100:] == SENTINEL).all()
        rc, got = ix.counts(capacity=99)
        assert rc == ERR_CAPACITY and b"capacity" in ix.L.bigsi_hip_last_error() and (got == SENTINEL).all()
        assert ix.L.bigsi_hip_column_popcounts(ix.ix, None, None, 100) == ERR_INVALID and ix.L.bigsi_hip_last_error()
    finally:
        ix.close()


@pytest.mark.parametrize("total", [300, 100])
def test_f_groups(total):
    """Three shards on one device: 300 columns -> 128 + 128 + 44 (uneven), 100 columns -> 64 + 36 + 0 (an empty shard); counts in global
    colour order, masked and unmasked, through HipHbmStorage.column_popcounts with every kind of mask it takes."""
    from bigsi_amd import _lib
    from bigsi_amd.bitrow import BitRow
    from bigsi_amd.storage import get_storage
    rng = np.random.default_rng(total)
    m = 2500
    st = get_storage({"storage-engine": "hip-hbm", "k": 31, "m": m, "h": 3,
                      "storage-config": {"name": "statsgrp%d" % next(_counter), "devices": [0, 0, 0], "max_cols": total}})
    st.delete_all()
    try:
        for key, v in (("number_of_rows", m), ("number_of_cols", total), ("ksi:bloomfilter_size", m), ("ksi:num_hashes", 3)):
            st.set_integer(key, v)
        bits = (rng.random((m, total)) < 0.3).astype(np.uint8)
        st.set_rows_packed(0, np.packbits(bits, axis=1))
        inf = st.res.info()
        sc = int(inf.shard_cols)
        assert inf.n_shards == 3 and ((total == 300 and 2 * sc < total < 3 * sc) or (total == 100 and total <= 2 * sc))
        got = st.column_popcounts()
        assert got.dtype == np.uint64 and got.shape == (total,) and np.array_equal(got, col_sums(bits))
        sel = rng.random(m) < 0.3
        by = pack_mask(sel, junk=True)
        for mask in (by, by.tobytes(), BitRow.frombytes(pack_mask(sel).tobytes(), m)):
            assert np.array_equal(st.column_popcounts(mask), col_sums(bits, sel))
        for bad in (by[:-1], by.tobytes() + b"\0", BitRow.frombytes(by.tobytes(), m - 1), by.astype(np.uint16)):
            with pytest.raises(ValueError):
                st.column_popcounts(bad)
        out = np.zeros(total, np.uint64)
        assert _lib.lib().bigsi_hip_group_column_popcounts(st.handle, None, ptr(out), total - 1) == ERR_CAPACITY
    finally:
        st.delete_all()


def test_h_view_handle():
    rng = np.random.default_rng(18)
    bits = (rng.random((3001, 77)) < 0.5).astype(np.uint8)
    ix = Raw(bits)
    view = C.c_void_p()
    ix.lib.check(ix.L.bigsi_hip_open_view(ix.ix, C.byref(view)))
    try:
        sel = rng.random(3001) < 0.5
        rc, got = ix.counts(handle=view)
        assert rc == 0 and np.array_equal(got, col_sums(bits))
        rc, got = ix.counts(pack_mask(sel), handle=view)
        assert rc == 0 and np.array_equal(got, col_sums(bits, sel))
    finally:
        ix.lib.check(ix.L.bigsi_hip_close(view))
        ix.close()


# --------------------------------------------------------------------------------------------- BIGSI level
K, M, H = 11, 4099, 3


def bits_of(bf):
    return np.unpackbits(np.frombuffer(bf.tobytes(), dtype=np.uint8))[:M].astype(bool)


def want_similar(filters, names, query_bits, leave_out=None):
    a = int(query_bits.sum())
    rows = []
    for c, name in enumerate(names):
        if name is None or c == leave_out:
            continue
        i, x = int((query_bits & filters[c]).sum()), int(filters[c].sum())
        u = a + x - i
        rows.append({"sample_name": name, "colour": c, "bits_shared": i, "jaccard": i / u if u else 0.0, "containment": i / a if a else 0.0})
    return sorted(rows, key=lambda r: -r["jaccard"])


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """Six samples, s1 and s2 sharing most of their sequence; their Bloom filters from BIGSI.bloom are the expected columns."""
    from bigsi_amd import BIGSI
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(2025)
    base = rand_seq(rng, 300)
    seqs = {"s0": rand_seq(rng, 200), "s1": base, "s2": base[:270] + rand_seq(rng, 30), "s3": rand_seq(rng, 400), "s4": rand_seq(rng, 40), "s5": rand_seq(rng, 300)}
    d = tmp_path_factory.mktemp("stats")
    c = {"storage-engine": "hip-hbm", "k": K, "m": M, "h": H, "storage-config": {"name": "stats%d" % next(_counter), "filename": str(d / "index.hbm")}}
    b = BIGSI.build_from_sequences(c, {n: [s] for n, s in seqs.items()})
    filters = [bits_of(BIGSI.bloom(c, list(seq_to_kmers(s, K)))) for s in seqs.values()]
    state = {"b": b, "cfg": c, "dir": d, "names": list(seqs), "filters": filters, "seqs": seqs}
    yield state
    b.delete()


def test_g_sample_stats_and_similar(small):
    import math
    from bigsi_amd import BIGSI
    from bigsi_amd.utils import seq_to_kmers
    b, names, filters = small["b"], small["names"], small["filters"]
    stats = b.sample_stats()
    assert [r["sample_name"] for r in stats] == names and [r["colour"] for r in stats] == list(range(6))
    for r, f in zip(stats, filters):
        x = int(f.sum())
        assert list(r) == ["sample_name", "colour", "bits_set", "fill", "kmer_fpr", "est_kmers"]
        assert type(r["bits_set"]) is int and r["bits_set"] == x and 0 < x < M
        assert r["fill"] == x / M and r["kmer_fpr"] == (x / M) ** H and r["est_kmers"] == -(M / H) * math.log1p(-x / M)
    # by name: the sample's own column is the mask and the sample is left out; its near-duplicate comes first
    got = b.similar_samples("s1")
    assert got == want_similar(filters, names, filters[1], leave_out=1)
    assert got[0]["sample_name"] == "s2" and got[0]["jaccard"] > 0.5 > got[1]["jaccard"] and len(got) == 5
    assert b.similar_samples("s1", limit=2) == got[:2]
    # by filter: the same numbers, the sample itself included (and first: Jaccard 1.0)
    bf = BIGSI.bloom(small["cfg"], list(seq_to_kmers(small["seqs"]["s1"], K)))
    with_self = b.similar_samples(bf)
    assert with_self == want_similar(filters, names, filters[1])
    assert with_self[0]["sample_name"] == "s1" and with_self[0]["jaccard"] == 1.0 and with_self[0]["containment"] == 1.0
    assert [r for r in with_self if r["colour"] != 1] == got
    assert b.similar_samples(bf.tobytes()) == with_self
    with pytest.raises(KeyError):
        b.similar_samples("no-such-sample")
    with pytest.raises(ValueError):
        b.similar_samples(BIGSI.bloom(dict(small["cfg"], m=M - 1), ["A" * K]))
    with pytest.raises(ValueError):
        b.similar_samples("s1", limit=0)
    # a deleted sample leaves both results; an inserted one appears in both
    b.delete_sample("s3")
    names2 = [None if n == "s3" else n for n in names]
    assert [r["sample_name"] for r in b.sample_stats()] == [n for n in names2 if n]
    assert b.similar_samples("s1") == want_similar(filters, names2, filters[1], leave_out=1)
    with pytest.raises(KeyError):
        b.similar_samples("s3")
    rng = np.random.default_rng(7)
    new_seq = small["seqs"]["s1"][:150] + rand_seq(rng, 100)
    nbf = BIGSI.bloom(small["cfg"], list(seq_to_kmers(new_seq, K)))
    b.insert(nbf, "s6")
    names3, filters3 = names2 + ["s6"], filters + [bits_of(nbf)]
    stats = b.sample_stats()
    assert stats[-1]["sample_name"] == "s6" and stats[-1]["colour"] == 6 and stats[-1]["bits_set"] == int(filters3[6].sum())
    assert b.similar_samples("s1") == want_similar(filters3, names3, filters3[1], leave_out=1)
    assert b.similar_samples("s6") == want_similar(filters3, names3, filters3[6], leave_out=6)
    small["names"], small["filters"] = names3, filters3


def test_cli_stats_and_similar(small, capsys):
    """`python -m bigsi_amd stats` in a process of its own on the index's snapshot; the other forms through the same main()."""
    from bigsi_amd.__main__ import main
    b, d = small["b"], small["dir"]
    b.storage.sync()
    cf = d / "config.yaml"
    cf.write_text(yaml.safe_dump(small["cfg"]))
    stats, sim = b.sample_stats(), b.similar_samples("s1")
    r = subprocess.run([sys.executable, "-m", "bigsi_amd", "stats", "--config", str(cf)], cwd=str(d), capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == json.dumps(stats) + "\n" and json.loads(r.stdout) == stats
    capsys.readouterr()
    assert main(["similar", "s1", "--config", str(cf)]) == 0
    assert capsys.readouterr().out == json.dumps(sim) + "\n"
    assert main(["similar", "s1", "--limit", "2", "--format", "csv", "--config", str(cf)]) == 0
    rows = list(csv.reader(io.StringIO(capsys.readouterr().out)))
    assert rows[0] == ["sample_name", "colour", "bits_shared", "jaccard", "containment"] and len(rows) == 3
    assert [(r_[0], int(r_[1]), int(r_[2]), float(r_[3]), float(r_[4])) for r_ in rows[1:]] == [tuple(x.values()) for x in sim[:2]]
    assert main(["stats", "--format", "csv", "--config", str(cf)]) == 0
    rows = list(csv.reader(io.StringIO(capsys.readouterr().out)))
    assert rows[0] == ["sample_name", "colour", "bits_set", "fill", "kmer_fpr", "est_kmers"] and len(rows) == len(stats) + 1
    assert [(r_[0], int(r_[1]), int(r_[2]), float(r_[3]), float(r_[4]), float(r_[5])) for r_ in rows[1:]] == [tuple(x.values()) for x in stats]
