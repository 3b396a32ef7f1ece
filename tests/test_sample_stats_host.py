"""Sample statistics without a GPU: the CPU twin of bigsi_hip_column_popcounts against numpy on the rows written, the derivation of
sample_stats / similar_samples on hand-made count arrays (bigsi_amd/stats.py), and the command line of `stats` and `similar`."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from raw_index import ptr

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_CAPACITY = -1, -5


@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    return L


def twin_index(L, bits):
    """A twin index holding the bit matrix `bits` (uint8[m, n] of 0 / 1), written through set_rows."""
    m, n = bits.shape
    ix = C.c_void_p()
    assert L.bigsi_cpu_open(C.c_uint64(m), C.c_uint64(n), C.c_uint64(n), C.c_uint32(3), 0, C.byref(ix)) == 0
    packed = np.ascontiguousarray(np.packbits(bits, axis=1))
    ids = np.arange(m, dtype=np.uint64)
    assert L.bigsi_cpu_set_rows(ix, ptr(ids), C.c_uint64(m), ptr(packed), C.c_uint64(packed.shape[1])) == 0, L.bigsi_cpu_last_error()
    return ix


def twin_counts(L, ix, n, mask=None, capacity=None):
    out = np.full(n, 0xDEAD, dtype=np.uint64)
    rc = L.bigsi_cpu_column_popcounts(ix, ptr(mask), ptr(out), C.c_uint64(n if capacity is None else capacity))
    return rc, out


def pack_mask(sel, junk=False):
    """Row selector (bool[m]) in the layout get_column writes; junk: every bit of the last byte past row m - 1 set."""
    m = sel.size
    by = np.packbits(sel.astype(np.uint8))
    if junk and m % 8:
        by[-1] |= (1 << (8 - m % 8)) - 1
    return np.ascontiguousarray(by)


def ragged_bits(m, n):
    """Shape C of the GPU suite: column c set in exactly the rows r < (c * 37) % (m + 1)."""
    return (np.arange(m)[:, None] < ((np.arange(n) * 37) % (m + 1))[None, :]).astype(np.uint8)


def test_twin_against_numpy_unmasked(cpu):
    rng = np.random.default_rng(1)
    for bits in [(rng.random((1009, 200)) < 0.3).astype(np.uint8)] + [ragged_bits(257, n) for n in (1, 8, 63, 64, 65, 127, 128, 129, 1023, 1025, 8191, 8193)]:
        ix = twin_index(cpu, bits)
        rc, got = twin_counts(cpu, ix, bits.shape[1])
        assert rc == 0, cpu.bigsi_cpu_last_error()
        assert np.array_equal(got, bits.sum(axis=0, dtype=np.uint64))
        assert cpu.bigsi_cpu_close(ix) == 0


def test_twin_masks_and_capacity(cpu):
    rng = np.random.default_rng(2)
    m, n = 1013, 300
    bits = (rng.random((m, n)) < 0.3).astype(np.uint8)
    ix = twin_index(cpu, bits)
    sel = rng.random(m) < 0.25
    want = bits[sel].sum(axis=0, dtype=np.uint64)
    rc, got = twin_counts(cpu, ix, n, pack_mask(sel))
    assert rc == 0 and np.array_equal(got, want)
    rc, got = twin_counts(cpu, ix, n, pack_mask(sel, junk=True))            # bits past row m - 1 are ignored
    assert rc == 0 and np.array_equal(got, want)
    rc, got = twin_counts(cpu, ix, n, pack_mask(np.ones(m, bool), junk=True))
    assert rc == 0 and np.array_equal(got, bits.sum(axis=0, dtype=np.uint64))
    rc, got = twin_counts(cpu, ix, n, pack_mask(np.zeros(m, bool)))
    assert rc == 0 and not got.any()
    rc, got = twin_counts(cpu, ix, n, capacity=n - 1)
    assert rc == ERR_CAPACITY and b"capacity" in cpu.bigsi_cpu_last_error() and (got == 0xDEAD).all()
    assert cpu.bigsi_cpu_column_popcounts(ix, None, None, C.c_uint64(n)) == ERR_INVALID
    assert cpu.bigsi_cpu_close(ix) == 0


def test_launch_shape_of_the_sweep(tmp_path):
    """plan_col_popcount (csrc/bigsi_launch.hpp, host-only): row blocks in whole mask words that cover every row once, counters that
    cannot wrap, whole flush periods that fit the planes, narrow indexes in workgroups of fewer wavefronts."""
    import subprocess
    src = tmp_path / "plan.cpp"
    src.write_text('#include "bigsi_launch.hpp"\n#include <cstdio>\n#include <cstdlib>\n'
                   'int main(int c, char **v) { for (int i = 1; i + 1 < c; i += 2) { auto p = bigsi::plan_col_popcount(strtoull(v[i], 0, 10), strtoull(v[i + 1], 0, 10));\n'
                   'printf("%u %llu %llu %llu %llu %u %llu %d %d\\n", p.block, (unsigned long long)p.seg_groups, (unsigned long long)p.rows_per_block, (unsigned long long)p.row_blocks,\n'
                   '(unsigned long long)p.grid, p.flush_groups, (unsigned long long)p.partial_stride, bigsi::kColPopPlanes, bigsi::kColPopLoads); } return 0; }\n')
    exe = str(tmp_path / "plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "bigsi_amd", "csrc"), "-o", exe, str(src)])
    shapes = [(1009, 16), (70001, 16), (257, 144), (10_000_000, 1568), (25_000_000, 992), (1 << 40, 16), (1, 16), (5000, 48)]
    out = subprocess.check_output([exe] + [str(x) for s in shapes for x in s], text=True).split("\n")
    for (m, stride), line in zip(shapes, out):
        block, seg_groups, rpb, rbs, grid, flush, pstride, planes, loads = (int(x) for x in line.split())
        segs = -(-stride // 128)
        assert block == 64 * min(segs, 4) and seg_groups * (block // 64) >= segs > (seg_groups - 1) * (block // 64)
        assert rpb % 64 == 0 and rpb * rbs >= m > rpb * (rbs - 1) and grid == seg_groups * rbs
        assert rpb <= 1 << 31                                   # a wavefront's 32-bit counters
        assert flush >= 1 and flush * loads <= 2 ** planes - 1      # rows between two flushes fit the planes
        assert rpb % (flush * loads) == 0 and rpb >= 2 * flush * loads   # no flush of a handful of rows at the end of a full block
        assert pstride == stride * 64
    # the shapes the design was sized for: a 100 k-sample index and a 62.5 k-sample shard both get a few thousand wavefronts
    for (m, stride) in shapes[3:5]:
        line = out[shapes.index((m, stride))].split()
        assert 2048 <= -(-stride // 128) * int(line[3]) <= 8192


# --------------------------------------------------------------------------------------------- derivation
def test_sample_stats_formulas():
    from bigsi_amd.stats import STATS_KEYS, derive_sample_stats
    m, h = 1000, 3
    counts = np.array([0, 250, 1000, 600, 999], dtype=np.uint64)
    names = ["empty", "quarter", "full", None, "nearly"]
    got = derive_sample_stats(counts, m, h, names)
    assert [r["colour"] for r in got] == [0, 1, 2, 4] and [r["sample_name"] for r in got] == ["empty", "quarter", "full", "nearly"]
    for r in got:
        assert tuple(r.keys()) == STATS_KEYS == ("sample_name", "colour", "bits_set", "fill", "kmer_fpr", "est_kmers")
        x = int(counts[r["colour"]])
        assert type(r["bits_set"]) is int and r["bits_set"] == x
        assert r["fill"] == x / m and r["kmer_fpr"] == (x / m) ** h
        assert r["est_kmers"] is None if x == m else r["est_kmers"] == -(m / h) * math.log1p(-x / m)
    assert got[0]["fill"] == 0.0 and got[0]["kmer_fpr"] == 0.0 and got[0]["est_kmers"] == 0.0
    assert got[2]["fill"] == 1.0 and got[2]["kmer_fpr"] == 1.0 and got[2]["est_kmers"] is None
    assert got[1]["est_kmers"] == pytest.approx(95.894, abs=1e-3)      # -(1000 / 3) * ln(0.75)
    json.dumps(got)


def test_similar_formulas_ties_and_limit():
    from bigsi_amd.stats import SIMILAR_KEYS, derive_similar
    counts = np.array([100, 50, 100, 0, 80, 100], dtype=np.uint64)
    masked = np.array([100, 25, 50, 0, 40, 50], dtype=np.uint64)
    names = ["self", "a", "b", "z", None, "c"]
    got = derive_similar(counts, 100, masked, names, leave_out=0)
    # jaccard: a 25 / 125 = 0.2, b 50 / 150 = 1/3, z 0 / 100 = 0, c 50 / 150 = 1/3: b before c (colour), then a, then z
    assert [r["sample_name"] for r in got] == ["b", "c", "a", "z"] and [r["colour"] for r in got] == [2, 5, 1, 3]
    for r in got:
        assert tuple(r.keys()) == SIMILAR_KEYS == ("sample_name", "colour", "bits_shared", "jaccard", "containment")
        i, x = int(masked[r["colour"]]), int(counts[r["colour"]])
        assert type(r["bits_shared"]) is int and r["bits_shared"] == i
        assert r["jaccard"] == i / (100 + x - i) and r["containment"] == i / 100
    assert derive_similar(counts, 100, masked, names, leave_out=0, limit=2) == got[:2]
    assert derive_similar(counts, 100, masked, names, leave_out=0, limit=99) == got
    with_self = derive_similar(counts, 100, masked, names)
    assert with_self[0] == {"sample_name": "self", "colour": 0, "bits_shared": 100, "jaccard": 1.0, "containment": 1.0} and with_self[1:] == got
    # an empty query filter (A == 0): nothing is shared, containment is 0.0 and not a division by zero; U == 0 for an empty sample
    empty = derive_similar(counts, 0, np.zeros(6, np.uint64), names)
    assert [r["colour"] for r in empty] == [0, 1, 2, 3, 5]
    assert all(r["jaccard"] == 0.0 and r["containment"] == 0.0 and r["bits_shared"] == 0 for r in empty)
    json.dumps(got)


def test_limit_is_validated_before_any_device_work():
    """similar_samples checks `limit` with check_limit before it touches its storage (there is none here)."""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    for bad, err in ((0, ValueError), (-3, ValueError), (2.0, TypeError), ("3", TypeError), (True, TypeError)):
        with pytest.raises(err):
            b.similar_samples("anything", limit=bad)


# --------------------------------------------------------------------------------------------- command line
def test_cli_parsing():
    from bigsi_amd.__main__ import build_parser
    p = build_parser()[0]
    a = p.parse_args(["stats", "--config", "c.yaml"])
    assert (a.cmd, a.config, a.format) == ("stats", "c.yaml", "json")
    assert p.parse_args(["stats", "-c", "c.yaml", "--format", "csv"]).format == "csv"
    a = p.parse_args(["similar", "S1", "--limit", "5", "--config", "c.yaml", "--format", "csv"])
    assert (a.cmd, a.sample, a.limit, a.config, a.format) == ("similar", "S1", 5, "c.yaml", "csv")
    a = p.parse_args(["similar", "S1"])
    assert a.limit is None and a.format == "json"
    for bad in (["similar"], ["similar", "S1", "--limit", "0"], ["stats", "--sharded"], ["similar", "S1", "--sharded"], ["stats", "--format", "tsv"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


class _FakeIndex(object):
    def sample_stats(self):
        from bigsi_amd.stats import derive_sample_stats
        return derive_sample_stats([10, 100], 100, 2, ["a", "b,c"])

    def similar_samples(self, sample, limit=None):
        from bigsi_amd.stats import derive_similar
        assert sample == "a"
        return derive_similar([10, 100, 40], 10, [10, 10, 0], ["a", "b,c", "d"], leave_out=0, limit=limit)


def test_cli_text_json_and_csv():
    import csv
    import io
    from bigsi_amd.__main__ import similar_text, stats_text
    ix = _FakeIndex()
    assert stats_text(ix) == json.dumps(ix.sample_stats())
    rows = list(csv.reader(io.StringIO(stats_text(ix, "csv"))))
    assert rows[0] == ["sample_name", "colour", "bits_set", "fill", "kmer_fpr", "est_kmers"]
    assert rows[1][:5] == ["a", "0", "10", "0.1", repr(0.1 ** 2)] and float(rows[1][5]) == -(100 / 2) * math.log1p(-0.1)
    assert rows[2] == ["b,c", "1", "100", "1.0", "1.0", ""]                     # None -> an empty field; the name is quoted
    assert similar_text(ix, "a") == json.dumps(ix.similar_samples("a"))
    assert json.loads(similar_text(ix, "a", limit=1)) == ix.similar_samples("a")[:1]
    rows = list(csv.reader(io.StringIO(similar_text(ix, "a", None, "csv"))))
    assert rows[0] == ["sample_name", "colour", "bits_shared", "jaccard", "containment"]
    assert rows[1] == ["b,c", "1", "10", "0.1", "1.0"] and rows[2] == ["d", "2", "0", "0.0", "0.0"]
