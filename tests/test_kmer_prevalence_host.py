"""K-mer prevalence without a GPU: the CPU twin of bigsi_hip_kmer_prevalence against numpy on a seeded bit matrix (row ids from the
oracle's hashing) and on the reference's own lookup outputs (G2), the ABI of the new headers, plan_kmer_prevalence
(csrc/bigsi_launch.hpp, compiled by g++), the host-only helpers of bigsi_amd/prevalence.py and the `prevalence` command on a stubbed
index."""
import csv
import ctypes as C
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from raw_index import ptr, rand_seq
from oracle import coracle

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
SENTINEL = 0xDEADBEEF


def pack(seqs):
    data = [s.encode("ascii") for s in seqs]
    off = np.zeros(len(data) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in data])
    return b"".join(data), off


@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    return L


def expected(bits, seqs, k, h, universe=None, subset=None):
    """numpy: per position the number of columns set in every one of the k-mer's h rows (row ids from the oracle's hashing), under
    the bool masks."""
    m, n = bits.shape
    u = np.ones(n, bool) if universe is None else universe
    tot, sub, off = [], [], [0]
    for s in seqs:
        for i in range(max(len(s) - k + 1, 0)):
            a = np.ones(n, bool)
            for r in coracle.kmer_rows(s[i:i + k], h, m):
                a &= bits[r].astype(bool)
            tot.append(int((a & u).sum()))
            if subset is not None:
                sub.append(int((a & u & subset).sum()))
        off.append(len(tot))
    return np.asarray(off, np.uint64), np.asarray(tot, np.uint32), (np.asarray(sub, np.uint32) if subset is not None else None)


def mask_bytes(flags, junk=True):
    """bool per column -> the row format; junk: every bit of the last byte past the last column set (must be ignored)."""
    by = np.packbits(flags.astype(np.uint8))
    if junk and flags.size % 8:
        by[-1] |= (1 << (8 - flags.size % 8)) - 1
    return np.ascontiguousarray(by)


class Twin(object):
    """A twin index holding the bit matrix `bits` (uint8[m, n]), written with bigsi_cpu_set_rows; `junk`: every bit of the row
    stride behind column n - 1 that set_rows takes is set."""

    def __init__(self, L, bits, h, junk=True):
        self.L, self.ix = L, C.c_void_p()
        self.m, self.n = bits.shape
        assert L.bigsi_cpu_open(C.c_uint64(self.m), C.c_uint64(self.n), C.c_uint64(self.n), C.c_uint32(h), 0, C.byref(self.ix)) == 0
        packed = np.packbits(bits, axis=1)
        if junk:
            wide = np.full((self.m, (self.n + 63) // 64 * 8), 0xFF, np.uint8)
            wide[:, :packed.shape[1]] = packed
            if self.n % 8:
                wide[:, packed.shape[1] - 1] |= (1 << (8 - self.n % 8)) - 1
            packed = wide
        packed = np.ascontiguousarray(packed)
        ids = np.arange(self.m, dtype=np.uint64)
        assert L.bigsi_cpu_set_rows(self.ix, ptr(ids), C.c_uint64(self.m), ptr(packed), C.c_uint64(packed.shape[1])) == 0, L.bigsi_cpu_last_error()

    def prevalence(self, seqs, k, universe=None, subset=None, capacity=None, want_sub=None, total_null=False):
        blob, off = pack(seqs)
        need = sum(max(len(s) - k + 1, 0) for s in seqs)
        pos = np.full(len(seqs) + 1, SENTINEL, np.uint64)
        tot = np.full(need + 3, SENTINEL, np.uint32)
        sub = np.full(need + 3, SENTINEL, np.uint32) if (subset is not None if want_sub is None else want_sub) else None
        rc = self.L.bigsi_cpu_kmer_prevalence(self.ix, blob, ptr(off), C.c_uint32(len(seqs)), C.c_uint32(k), ptr(universe), ptr(subset), ptr(pos),
                                              None if total_null else ptr(tot), ptr(sub), C.c_uint64(need if capacity is None else capacity))
        return rc, pos, tot, sub

    def close(self):
        assert self.L.bigsi_cpu_close(self.ix) == 0


# --------------------------------------------------------------------------------------------- the CPU twin
def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_twin_against_numpy(cpu):
    rng = np.random.default_rng(101)
    m, n, h, k = 509, 77, 3, 7
    bits = (rng.random((m, n)) < 0.6).astype(np.uint8)
    ix = Twin(cpu, bits, h)
    a = rand_seq(rng, 40)
    seqs = [a + a[5:25] + revcomp(a[:k]),          # repeated k-mers, and a k-mer together with its reverse complement
            rand_seq(rng, k),                      # exactly k characters
            rand_seq(rng, k - 1),                  # shorter than k
            rand_seq(rng, 23)]
    universe = rng.random(n) < 0.7
    inside = universe & (rng.random(n) < 0.5)
    outside = rng.random(n) < 0.5                  # not contained in the universe
    for uni, sub in ((None, None), (universe, None), (None, inside), (universe, inside), (universe, outside)):
        want = expected(bits, seqs, k, h, uni, sub)
        rc, pos, tot, got_sub = ix.prevalence(seqs, k, None if uni is None else mask_bytes(uni), None if sub is None else mask_bytes(sub))
        assert rc == 0, cpu.bigsi_cpu_last_error()
        assert np.array_equal(pos, want[0]) and np.array_equal(tot[:-3], want[1]) and (tot[-3:] == SENTINEL).all()
        if sub is not None:
            assert np.array_equal(got_sub[:-3], want[2]) and (got_sub[-3:] == SENTINEL).all()
    # the positions of a repeated k-mer carry the same numbers; the reverse complement shares its rows
    want = expected(bits, seqs, k, h)
    assert want[1][5] == want[1][40] and want[1][0] == want[1][len(seqs[0]) - k]
    assert want[1].max() > 0 and len(set(want[1].tolist())) > 3          # (the matrix is dense enough for the counts to differ)
    # errors
    rc, pos, tot, _ = ix.prevalence(seqs, k, capacity=int(want[0][-1]) - 1)
    assert rc == ERR_CAPACITY and np.array_equal(pos, want[0]) and (tot == SENTINEL).all()
    assert ix.prevalence(seqs, k, total_null=True)[0] == ERR_INVALID
    assert ix.prevalence(seqs, k, subset=None, want_sub=True)[0] == ERR_INVALID
    assert ix.prevalence(seqs, k, subset=mask_bytes(inside), want_sub=False)[0] == ERR_INVALID
    assert ix.prevalence(seqs, 0)[0] == ERR_INVALID
    ix.close()


def test_twin_on_the_reference_lookups(cpu):
    """G2: the reference's own lookup outputs -- a k-mer's total is the number of 1s in its bit string (its assertion: ATC in both
    samples, ATT and TTT in one each)."""
    from test_cpu_twin import Index
    seen = {}
    for g in load_golden("g2_lookup.json"):
        ix = Index(cpu, g["m"], g["h"], 64)
        for c, s in enumerate(g["samples"]):
            ix.add_sample(c, [s] if isinstance(s, str) else list(s), g["k"])
        for lk in g["lookups"]:
            kmers = [lk["kmers"]] if isinstance(lk["kmers"], str) else list(lk["kmers"])
            if any(len(km) != g["k"] for km in kmers):
                continue
            blob, off = pack(kmers)
            pos, tot = np.zeros(len(kmers) + 1, np.uint64), np.zeros(len(kmers), np.uint32)
            ix.ok(cpu.bigsi_cpu_kmer_prevalence(ix.ix, blob, ptr(off), C.c_uint32(len(kmers)), C.c_uint32(g["k"]), None, None, ptr(pos), ptr(tot), None,
                                                C.c_uint64(len(kmers))))
            assert pos.tolist() == list(range(len(kmers) + 1))
            for km, t in zip(kmers, tot):
                assert int(t) == lk["result"][km].count("1"), (km, lk)
                seen[km] = int(t)
        ix.close()
    assert seen["ATC"] == 2 and seen["ATT"] == 1 and seen["TTT"] == 1 and seen["GGG"] == 0


# --------------------------------------------------------------------------------------------- the ABI
def header_names(name, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % prefix, src)))


def test_abi_of_the_new_headers(tmp_path):
    from bigsi_amd import _lib
    new = ["bigsi_hip_batch_kmer_prevalence", "bigsi_hip_kmer_prevalence"]
    assert header_names("bigsi_hip_prevalence.h", "bigsi_hip_") == sorted(_lib.PREVALENCE_SIGNATURES) == new
    for name in new:
        assert name not in _lib.SIGNATURES and name not in _lib.COMPACT_SIGNATURES and name not in _lib.FOLD_SIGNATURES
    for other in ("bigsi_hip.h", "bigsi_hip_compact.h", "bigsi_hip_fold.h", "bigsi_hip_group.h", "bigsi_hip_testing.h", "bigsi_hip_text.h"):
        assert not set(new) & set(header_names(other, "bigsi_hip_")), other
    # the parameter counts of the binding are the header's
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)      # noqa: E731
    decl = lambda src, prefix: {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\b%s(\w+)\s*\(([^;{]*?)\)\s*;" % prefix, src)}      # noqa: E731
    cpu_h, hip_h = open(os.path.join(ROOT, "include", "bigsi_cpu_prevalence.h")).read(), open(os.path.join(ROOT, "include", "bigsi_hip_prevalence.h")).read()
    c, h = decl(strip(cpu_h), "bigsi_cpu_"), decl(strip(hip_h), "bigsi_hip_")
    for name in new:
        assert len(h[name[len("bigsi_hip_"):]].split(",")) == len(_lib.PREVALENCE_SIGNATURES[name][1])
    # the twin mirrors the one-shot call (it has no batch objects): the same parameter list, the renaming macro, the exported symbol
    assert sorted(c) == ["kmer_prevalence"] and sorted(h) == ["batch_kmer_prevalence", "kmer_prevalence"]
    assert c["kmer_prevalence"].replace("bigsi_cpu_index", "bigsi_hip_index") == h["kmer_prevalence"]
    assert "#define bigsi_hip_kmer_prevalence bigsi_cpu_kmer_prevalence" in cpu_h and "BIGSI_USE_CPU_TWIN" in cpu_h
    assert "bigsi_hip_batch_kmer_prevalence" in strip(hip_h) and "no twin of bigsi_hip_batch_kmer_prevalence" in cpu_h
    assert hasattr(C.CDLL(LIB), "bigsi_cpu_kmer_prevalence")
    # both headers are C99
    for hdr in ("bigsi_hip_prevalence.h", "bigsi_cpu_prevalence.h"):
        src = tmp_path / ("use_%s.c" % hdr[:-2])
        src.write_text('#include "%s"\nint main(void) { return bigsi_hip_kmer_prevalence(0, 0, 0, 1, 3, 0, 0, 0, 0, 0, 0) == BIGSI_OK; }\n' % hdr)
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_binds_the_new_symbols():
    """The device library exports what the header declares, with the binding's argument types (loading it needs no GPU)."""
    from bigsi_amd import _lib
    for name, (res, args) in _lib.PREVALENCE_SIGNATURES.items():
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == args and fn.restype == res


# --------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("prevalence_host") / "libprevalence_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "prevalence_host.cpp")])
    return C.CDLL(so)


PLAN_KEYS = ("block", "segs", "slices", "segs_per_slice", "waves_per_slice", "waves", "grid", "segs_per_step", "loads_per_step", "partial_stride",
             "partial_entries", "loads", "max_loads", "target")


def plan(lib, total_pos, total_unique, wv, h):
    out = np.zeros(14, np.uint64)
    lib.prevalence_host_plan(C.c_uint64(total_pos), C.c_uint64(total_unique), C.c_uint64(wv), C.c_uint32(h), ptr(out))
    return dict(zip(PLAN_KEYS, (int(x) for x in out)))


def check_plan(p, total_pos, total_unique, wv, h):
    segs = max(-(-wv // 128), 1)
    assert p["segs"] == segs and p["loads"] == 8 and p["max_loads"] == 16 and p["target"] == 4096
    # the slices cover [0, segs) exactly once and none is empty
    assert 1 <= p["slices"] <= segs
    cover = [(s * p["segs_per_slice"], min((s + 1) * p["segs_per_slice"], segs)) for s in range(p["slices"])]
    assert cover[0][0] == 0 and cover[-1][1] == segs and all(a < b for a, b in cover) and all(cover[i][1] == cover[i + 1][0] for i in range(len(cover) - 1))
    # one slice per k-mer once there are enough k-mers; never more items than needed to reach the target, give or take the rounding
    if total_unique >= p["target"] or segs == 1:
        assert p["slices"] == 1
    else:
        assert p["slices"] <= min(segs, -(-p["target"] // max(total_unique, 1)))
    # loads in flight: at most 16, and 8 wherever the step has that much work
    assert p["loads_per_step"] <= p["max_loads"]
    assert p["loads_per_step"] >= min(8, h * p["segs_per_slice"])
    assert p["segs_per_step"] * min(h, 8) <= p["max_loads"] and p["segs_per_step"] == (1 if h >= 8 else -(-8 // h))
    # every slot has a wavefront in every slice; the grid holds them all and fits 31 bits
    assert p["waves"] == p["waves_per_slice"] * p["slices"] and p["waves_per_slice"] <= max(total_pos, 0)
    assert (p["waves_per_slice"] > 0) == (total_pos > 0)
    assert p["waves"] <= 2 * p["target"] + p["slices"]
    assert p["block"] in (64, 128, 192, 256) and p["block"] == min(segs, 4) * 64
    assert p["grid"] * (p["block"] // 64) >= p["waves"] and p["grid"] < 1 << 31 and (p["grid"] - 1) * (p["block"] // 64) < max(p["waves"], 1)
    # the partial array: an entry per slice and slot
    assert p["partial_stride"] == total_pos and p["partial_entries"] == p["slices"] * total_pos


def test_plan_pinned_shapes(plan_lib):
    # one 1 kbp query on 100 k samples (1563 words, 13 segments): sliced five ways, a wavefront per (slot, slice)
    p = plan(plan_lib, 970, 970, 1563, 4)
    check_plan(p, 970, 970, 1563, 4)
    assert (p["slices"], p["segs_per_slice"], p["waves_per_slice"], p["waves"], p["block"], p["grid"]) == (5, 3, 970, 4850, 256, 1213)
    assert (p["segs_per_step"], p["loads_per_step"]) == (2, 8)
    # the headline batch, 8192 x 970 k-mers: one slice, 4096 wavefronts striding
    p = plan(plan_lib, 8192 * 970, 8192 * 970, 1563, 4)
    check_plan(p, 8192 * 970, 8192 * 970, 1563, 4)
    assert (p["slices"], p["segs_per_slice"], p["waves_per_slice"], p["waves"], p["grid"]) == (1, 13, 4096, 4096, 1024)
    assert p["partial_entries"] == 8192 * 970
    # one read (31 k-mers of 61 bp) on 10 k samples (157 words, 2 segments)
    p = plan(plan_lib, 31, 31, 157, 3)
    check_plan(p, 31, 31, 157, 3)
    assert (p["slices"], p["segs_per_slice"], p["waves_per_slice"], p["block"], p["grid"], p["segs_per_step"], p["loads_per_step"]) == (2, 1, 31, 128, 31, 3, 3)
    # a one-word index: one segment, one slice, one wavefront per workgroup
    p = plan(plan_lib, 970, 900, 1, 3)
    check_plan(p, 970, 900, 1, 3)
    assert (p["segs"], p["slices"], p["block"], p["waves"], p["grid"], p["loads_per_step"]) == (1, 1, 64, 970, 970, 3)
    # nothing to sweep
    p = plan(plan_lib, 0, 0, 1563, 4)
    check_plan(p, 0, 0, 1563, 4)
    assert p["grid"] == 0 and p["waves"] == 0 and p["partial_entries"] == 0
    # a run-time h: one segment per step, its rows in groups of eight
    p = plan(plan_lib, 5000, 5000, 1563, 9)
    assert (p["segs_per_step"], p["loads_per_step"]) == (1, 8)


def test_plan_invariants_over_seeded_shapes(plan_lib):
    rng = np.random.default_rng(77)
    for _ in range(4000):
        total_pos = int(rng.choice([0, 1, 2, 31, 970, 4095, 4096, 4097, 8191, 8193, int(rng.integers(1, 1 << 24))]))
        total_unique = int(rng.integers(0, total_pos + 1)) if total_pos else 0
        if total_pos and total_unique == 0:
            total_unique = 1
        wv = int(rng.choice([0, 1, 2, 127, 128, 129, 157, 1563, 977, int(rng.integers(1, 1 << 20)), (1 << 26) - 1]))
        h = int(rng.integers(1, 13))
        check_plan(plan(plan_lib, total_pos, total_unique, wv, h), total_pos, total_unique, wv, h)


# --------------------------------------------------------------------------------------------- bigsi_amd/prevalence.py
def test_masks():
    from bigsi_amd.graph.metadata import DELETION_SPECIAL_SAMPLE_NAME as DEL
    from bigsi_amd.prevalence import pack_mask, subset_mask, universe_mask
    names = ["a", "b", DEL, "d", None, "f", "g", "h", "i"]
    named = np.asarray([n is not None and n != DEL for n in names])
    # the matrix as wide as the metadata: deleted colours out of the universe
    mask, n = universe_mask(9, names)
    assert n == 7 and np.array_equal(mask, np.packbits(named)) and mask.dtype == np.uint8 and mask.size == 2
    # a matrix WIDER than the metadata (21 columns, 9 records): masks of the matrix's width, the columns without a record in no universe
    mask, n = universe_mask(21, names)
    flags = np.zeros(21, bool)
    flags[:9] = named
    assert n == 7 and np.array_equal(mask, np.packbits(flags)) and mask.size == 3
    # ... and a narrower one: names beyond it name no column
    mask, n = universe_mask(6, names)
    assert n == 4 and np.array_equal(mask, np.packbits(named[:6]))
    mask, n = universe_mask(16, ["x"] * 16)
    assert n == 16 and mask.tolist() == [255, 255]
    assert universe_mask(0, [])[0].tolist() == [0] and pack_mask([]).tolist() == [0]
    mask, n = subset_mask(21, names, ["i", "b", "a"])
    flags = np.zeros(21, bool)
    flags[[0, 1, 8]] = True
    assert n == 3 and np.array_equal(mask, np.packbits(flags)) and mask.size == 3
    for bad in ("zz", DEL, "c"):
        with pytest.raises(ValueError) as e:
            subset_mask(9, names, ["a", bad])
        assert repr(bad) in str(e.value)
    with pytest.raises(ValueError) as e:
        subset_mask(6, names, ["a", "i"])          # colour 8 is not in a matrix of 6 columns
    assert "'i'" in str(e.value)
    with pytest.raises(ValueError) as e:
        subset_mask(9, names, ["a", "b", "a"])
    assert "'a'" in str(e.value)
    with pytest.raises(ValueError):
        subset_mask(9, names, [])
    with pytest.raises(TypeError):
        subset_mask(9, names, "a")


def test_record_assembly_and_csv():
    from bigsi_amd.prevalence import CSV_KEYS, RECORD_KEYS, assemble, to_csv
    seqs = ["ACGTAC", "AC", "ACGACG"]          # k = 3: 4 positions, none, 4 positions of which 3 are distinct strings
    pos = np.asarray([0, 4, 4, 8], np.uint64)
    total = np.asarray([5, 4, 3, 2, 9, 8, 7, 9], np.uint32)
    sub = np.asarray([1, 0, 1, 0, 2, 2, 1, 2], np.uint32)
    recs = assemble(seqs, 3, pos, total, sub, 10, 2)
    assert [tuple(r) for r in recs] == [RECORD_KEYS] * 3
    assert recs[0] == {"num_kmers": 4, "num_unique": 4, "num_samples": 10, "subset_size": 2, "samples_with_kmer": [5, 4, 3, 2], "subset_with_kmer": [1, 0, 1, 0]}
    assert recs[1] == {"num_kmers": 0, "num_unique": 0, "num_samples": 10, "subset_size": 2, "samples_with_kmer": [], "subset_with_kmer": []}
    assert recs[2]["num_unique"] == 3 and recs[2]["samples_with_kmer"] == [9, 8, 7, 9]
    assert all(type(x) is int for r in recs for x in r["samples_with_kmer"] + r["subset_with_kmer"])
    json.dumps(recs)
    plain = assemble(seqs, 3, pos, total, None, 10, None)
    assert plain[0]["subset_size"] is None and plain[0]["subset_with_kmer"] is None and plain[2]["samples_with_kmer"] == [9, 8, 7, 9]
    with pytest.raises(ValueError):
        assemble(seqs, 3, np.asarray([0, 3, 4, 8], np.uint64), total, None, 10, None)
    rows = list(csv.reader(io.StringIO(to_csv(recs, seqs, 3))))
    assert tuple(rows[0]) == CSV_KEYS == ("record", "pos", "kmer", "samples", "in_subset") and len(rows) == 9
    assert rows[1] == ["0", "0", "ACG", "5", "1"] and rows[4] == ["0", "3", "TAC", "2", "0"] and rows[5] == ["2", "0", "ACG", "9", "2"]
    rows = list(csv.reader(io.StringIO(to_csv(plain, seqs, 3))))
    assert rows[1] == ["0", "0", "ACG", "5", ""]
    from bigsi_amd.utils import seq_to_kmers
    assert [r[2] for r in rows[1:5]] == list(seq_to_kmers(seqs[0], 3))          # kmer: the text as seq_to_kmers yields it


# --------------------------------------------------------------------------------------------- the command
class StubIndex(object):
    """What prevalence_text needs of a BIGSI: kmer_size and kmer_prevalence_many (position p of a query counts p + len(query))."""
    kmer_size = 3

    def __init__(self):
        self.calls = []

    def kmer_prevalence_many(self, seqs, samples=None):
        self.calls.append((list(seqs), samples))
        out = []
        for s in seqs:
            n = max(len(s) - 2, 0)
            out.append({"num_kmers": n, "num_unique": n, "num_samples": 50, "subset_size": len(samples) if samples else None,
                        "samples_with_kmer": [p + len(s) for p in range(n)], "subset_with_kmer": [p for p in range(n)] if samples else None})
        return out


def test_cli_parsing_and_text(tmp_path, monkeypatch, capsys):
    import bigsi_amd.__main__ as cli
    p = cli.build_parser()[0]
    a = p.parse_args(["prevalence", "ACGT", "-s", "x", "-s", "y", "--format", "csv", "--config", "c.yaml"])
    assert (a.cmd, a.seq, a.fasta, a.samples, a.samples_file, a.format) == ("prevalence", "ACGT", None, ["x", "y"], None, "csv")
    a = p.parse_args(["prevalence", "--fasta", "q.fa", "--samples-file", "names.txt", "--config", "c.yaml"])
    assert (a.seq, a.fasta, a.samples, a.samples_file, a.format) == (None, "q.fa", [], "names.txt", "json")
    # text from a stubbed index
    ix = StubIndex()
    text = cli.prevalence_text(ix, ["ACGTA", "AC"], None, "json")
    got = json.loads(text)
    assert [list(r)[0] for r in got] == ["query", "query"] and got[0]["query"] == "ACGTA" and got[0]["samples_with_kmer"] == [5, 6, 7]
    assert got[0]["subset_with_kmer"] is None and got[1]["num_kmers"] == 0 and ix.calls == [(["ACGTA", "AC"], None)]
    rows = list(csv.reader(io.StringIO(cli.prevalence_text(ix, ["ACGTA", "AC", "GGGG"], ["x"], "csv"))))
    assert rows[0] == ["record", "pos", "kmer", "samples", "in_subset"]
    assert rows[1:] == [["0", "0", "ACG", "5", "0"], ["0", "1", "CGT", "6", "1"], ["0", "2", "GTA", "7", "2"], ["2", "0", "GGG", "4", "0"], ["2", "1", "GGG", "5", "1"]]
    # a FASTA file goes out in bounded device calls, results in input order
    ix = StubIndex()
    monkeypatch.setattr(cli, "PREVALENCE_BATCH_POSITIONS", 5)
    got = json.loads(cli.prevalence_text(ix, ["ACGTA", "ACGT", "ACGTACGTAC", "AC", "ACG"], None, "json"))
    assert [c[0] for c in ix.calls] == [["ACGTA", "ACGT"], ["ACGTACGTAC"], ["AC", "ACG"]]
    assert [r["query"] for r in got] == ["ACGTA", "ACGT", "ACGTACGTAC", "AC", "ACG"] and [r["num_kmers"] for r in got] == [3, 2, 8, 0, 1]
    # refusals, before any index is opened
    cf = tmp_path / "c.yaml"
    cf.write_text("k: 3\nm: 100\nh: 2\nstorage-engine: hip-hbm\nstorage-config: {name: never-opened}\n")
    for argv, word in ((["prevalence", "ACGT", "--sharded", "--config", str(cf)], "--sharded"),
                       (["prevalence", "--config", str(cf)], "SEQ or --fasta"),
                       (["prevalence", "ACGT", "--fasta", "q.fa", "--config", str(cf)], "SEQ or --fasta")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_group_indexes_are_refused():
    """devices=[...] indexes: refused in Python before the device is asked (the per-shard sweep is a follow-up)."""
    from bigsi_amd._lib import ERR_STATE, BigsiHipError
    from bigsi_amd.graph.bigsi import BIGSI
    from bigsi_amd.storage.hip_hbm import HipHbmStorage

    class Res(object):
        is_group = True

    for obj, call in ((BIGSI.__new__(BIGSI), lambda o: o.kmer_prevalence_many(["ACGT"])), (HipHbmStorage.__new__(HipHbmStorage), lambda o: o.kmer_prevalence(["ACGT"], 3))):
        if isinstance(obj, BIGSI):
            obj.storage = HipHbmStorage.__new__(HipHbmStorage)
            obj.storage.res = Res()
        else:
            obj.res = Res()
        with pytest.raises(BigsiHipError) as e:
            call(obj)
        assert e.value.code == ERR_STATE and "multi-GPU" in str(e.value)
    with pytest.raises(ValueError):
        o = BIGSI.__new__(BIGSI)
        o.storage = HipHbmStorage.__new__(HipHbmStorage)
        o.storage.res = type("R", (), {"is_group": False})()
        o.kmer_prevalence("ACGéT")
