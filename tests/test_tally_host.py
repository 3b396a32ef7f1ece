"""Query-set tally without a GPU: the host planners plan_tally / plan_tally_chunks (csrc/bigsi_launch.hpp, compiled by g++) against a
plain Python restatement (tests/tally_ref.py) and their own invariants -- every chunk within its three bounds, the chunks covering the
input once and in order, a sequence beyond a bound a chunk of its own --, the CPU twin bigsi_cpu_search_tally against numpy
(oracle.coracle's hashing plus the row bytes) on the planted indexes the GPU tests use, the conditions those indexes must hold so that
no GPU comparison passes vacuously, the host layer (bigsi_amd/tally.py: order, ties, limit, deleted samples, JSON / CSV), what
BIGSI.tally and the command line decide before any device call, and a stand-alone sanitized program over the planners and the twin."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import tally_ref as T
from conftest import ROOT
from raw_index import ptr

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
WIDTHS = (1, 63, 64, 65, 127, 129, 200, 775)          # 775: 13 result words, more than one workgroup's four
TILE_SEQS = (1, 63, 64, 65, T.TILE - 1, T.TILE, T.TILE + 1)


# --------------------------------------------------------------------------------------------- the planners
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tally_host") / "libtally_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "tally_host.cpp")])
    lib = C.CDLL(so)
    lib.tally_host_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    lib.tally_host_chunks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.tally_host_chunks.restype = C.c_uint64
    return lib


def compiled_plan(lib, n_seqs, wv):
    out = np.zeros(7, np.uint64)
    lib.tally_host_plan(n_seqs, wv, ptr(out))
    return dict(zip(("block", "tile", "word_groups", "tiles", "grid", "totals_grid", "too_large"), (int(x) for x in out)))


def compiled_chunks(lib, lengths, k, wv_pad, count_bytes):
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.uint64))]).astype(np.uint64)
    cuts = np.zeros(len(lengths) + 2, np.uint64)
    n = lib.tally_host_chunks(ptr(off), len(lengths), k, wv_pad, count_bytes, ptr(cuts), cuts.size)
    assert 2 <= n <= cuts.size
    return [int(x) for x in cuts[:n]]


def test_constants_are_the_restated_ones(plan_lib):
    c = np.zeros(7, np.uint64)
    plan_lib.tally_host_constants(ptr(c))
    assert [int(x) for x in c] == [T.BLOCK, T.TILE, T.LOADS, T.TOTALS_TILE, T.CHUNK_SEQS, T.CHUNK_POSITIONS, T.COUNTER_BYTES]
    header = open(os.path.join(ROOT, "include", "bigsi_hip_tally.h")).read()
    for name, value in (("BIGSI_TALLY_CHUNK_SEQS", "4096u"), ("BIGSI_TALLY_CHUNK_POSITIONS", "(1u << 20)"), ("BIGSI_TALLY_COUNTER_BYTES", "(2ull << 30)")):
        assert "#define %s %s" % (name, value) in header
    assert (T.CHUNK_SEQS, T.CHUNK_POSITIONS, T.COUNTER_BYTES) == (4096, 1 << 20, 2 << 30)
    assert T.TILE % T.LOADS == 0 and T.BLOCK % 64 == 0


def test_plan_tally_against_restatement(plan_lib):
    for n_seqs in (1, 2, 63, 64, 65, T.TILE - 1, T.TILE, T.TILE + 1, 4095, 4096, 4097, 8192, 0xFFFFFFFF):
        for wv in (1, 2, 3, 4, 5, 13, 1563, 1 << 20, 1 << 26):
            p = compiled_plan(plan_lib, n_seqs, wv)
            assert p == T.plan_tally(n_seqs, wv), (n_seqs, wv)
            # every (word, query) pair belongs to exactly one wavefront of the grid
            assert (p["word_groups"] - 1) * (p["block"] // 64) < wv <= p["word_groups"] * (p["block"] // 64)
            assert (p["tiles"] - 1) * p["tile"] < n_seqs <= p["tiles"] * p["tile"]
            assert (p["totals_grid"] - 1) * T.TOTALS_TILE < n_seqs <= p["totals_grid"] * T.TOTALS_TILE
            assert (p["too_large"] != 0) == (p["grid"] > 0x7FFFFFFF)
    assert compiled_plan(plan_lib, 0xFFFFFFFF, 1 << 26)["too_large"] and not compiled_plan(plan_lib, 8192, 1563)["too_large"]


def check_chunks(cuts, lengths, k, wv_pad, count_bytes):
    n = len(lengths)
    assert cuts[0] == 0 and cuts[-1] == n and all(a < b for a, b in zip(cuts, cuts[1:]))          # once, in order, none empty
    for a, b in zip(cuts, cuts[1:]):
        pos = sum(max(x - k + 1, 0) for x in lengths[a:b])
        assert b - a <= T.CHUNK_SEQS
        assert b - a == 1 or (pos <= T.CHUNK_POSITIONS and (b - a) * wv_pad * 64 * count_bytes <= T.COUNTER_BYTES), (a, b, pos)


def test_plan_tally_chunks_against_restatement(plan_lib):
    rng = np.random.default_rng(5)
    k = 31
    narrow, wide = 2, 100_000 // 64 + 2                          # wide: 4096 sequences x 1564 words x 64 x 4 bytes = 1.5 GiB, inside the budget
    binding = 1 << 15                                            # 2 GiB / (32768 x 64 x 4) = 256 sequences: the budget binds before 4096
    shapes = []
    for n in (1, 4095, 4096, 4097, 9000):
        shapes.append(([int(x) for x in rng.integers(0, 200, n)], narrow, 4))
        shapes.append(([int(x) for x in rng.integers(0, 200, n)], wide, 4))
        shapes.append(([int(x) for x in rng.integers(0, 200, n)], binding, 4))
        shapes.append(([int(x) for x in rng.integers(0, 200, n)], binding, 2))
        shapes.append(([int(x) for x in rng.integers(0, 200, n)], binding, 0))          # an exact stream: no counters, no byte bound
    per = 2000
    straddle = [per + k - 1] * 600                               # 2^20 / 2000 = 524.3: the cut falls inside sequence 524
    shapes += [(straddle, narrow, 4), (straddle[:524], narrow, 4), (straddle[:525], narrow, 4)]
    exact_fit = [1024 + k - 1] * 2048                            # 1024 sequences reach 2^20 exactly
    shapes.append((exact_fit, narrow, 0))
    giant = list(straddle)
    giant[3] = (1 << 20) + 500 + k - 1                           # one sequence beyond the position bound
    shapes.append((giant, narrow, 4))
    shapes.append(([10] * 50, narrow, 4))                        # nothing but sequences shorter than k
    shapes.append(([100], 1 << 26, 4))                           # one sequence whose counters alone pass the budget
    for lengths, wv_pad, cb in shapes:
        cuts = compiled_chunks(plan_lib, lengths, k, wv_pad, cb)
        assert cuts == T.plan_tally_chunks(lengths, k, wv_pad, cb), (len(lengths), wv_pad, cb)
        check_chunks(cuts, lengths, k, wv_pad, cb)
    # the pinned cuts
    assert compiled_chunks(plan_lib, [100] * 4096, k, narrow, 4) == [0, 4096] and compiled_chunks(plan_lib, [100] * 4097, k, narrow, 4) == [0, 4096, 4097]
    assert compiled_chunks(plan_lib, [100] * 4095, k, narrow, 4) == [0, 4095] and compiled_chunks(plan_lib, [100], k, narrow, 4) == [0, 1]
    assert compiled_chunks(plan_lib, straddle, k, narrow, 4) == [0, 524, 600] and compiled_chunks(plan_lib, straddle[:524], k, narrow, 4) == [0, 524]
    assert compiled_chunks(plan_lib, exact_fit, k, narrow, 0) == [0, 1024, 2048]
    assert compiled_chunks(plan_lib, giant, k, narrow, 4)[:4] == [0, 3, 4, 528]          # the giant alone in [3, 4)
    assert compiled_chunks(plan_lib, [100] * 600, k, binding, 4) == [0, 256, 512, 600] and compiled_chunks(plan_lib, [100] * 600, k, binding, 2) == [0, 512, 600]
    assert compiled_chunks(plan_lib, [100] * 600, k, binding, 0) == [0, 600]
    assert compiled_chunks(plan_lib, [100] * 3, k, 1 << 26, 4) == [0, 1, 2, 3]


def test_the_stream_case_is_cut_as_the_gpu_test_needs(plan_lib):
    lengths = T.stream_lengths()
    for cb in (0, 4):
        assert compiled_chunks(plan_lib, lengths, T.K, 4, cb) == [0, 5, 6, 12]


# --------------------------------------------------------------------------------------------- the reference's own conditions
@pytest.mark.parametrize("n_cols", WIDTHS)
def test_width_cases_cannot_pass_vacuously(n_cols):
    p = T.planted(n_cols, 9)
    thr, i, e = p.edge_threshold()
    assert 0 < thr < 1 and T.min_kmers(int(p.us[i]), thr) == int(p.counts[i, e]) < p.us[i]          # `>=` hits it, `>` would not
    assert set(p.edges) == {c for c in (0, 63, 64, n_cols - 1, 64 * ((n_cols - 1) // 64)) if 0 <= c < n_cols}
    for t in (1.0, thr):
        T.check_conditions(p, t)
    qh1, kf1, tot1 = p.tally(1.0)
    qht, kft, tott = p.tally(thr)
    assert (qht >= qh1).all() and (qht > qh1).any() and int(tott[3]) >= int(tot1[3])
    hit1 = qh1 > 0                                              # at threshold 1 a hit found every k-mer of its query
    assert np.array_equal(kf1[hit1] > 0, hit1[hit1]) and int(tot1[0]) == 8 and int(tot1[2]) == 1 and int(tot1[1]) == int(p.us.sum())


@pytest.mark.parametrize("n_seqs", TILE_SEQS)
def test_tile_cases_cannot_pass_vacuously(n_seqs):
    p = T.planted(200, n_seqs, seed=n_seqs)
    assert T.plan_tally(n_seqs, 4)["tile"] == T.TILE
    if n_seqs >= 3:
        for t in (1.0, p.edge_threshold()[0]):
            T.check_conditions(p, t)
    else:
        assert p.tally(1.0)[0][0] == 1                          # column 0 holds every k-mer of the only query


def test_tally_of_is_the_definition():
    p = T.planted(129, 9)
    thr = p.edge_threshold()[0]
    for t in (1.0, thr, 0.0, -0.5):
        qh, kf, totals = np.zeros(129, np.uint64), np.zeros(129, np.uint64), np.zeros(4, np.uint64)
        for u, c in zip(p.us, p.counts):
            if u == 0:
                totals[2] += 1
                continue
            mk = T.min_kmers(int(u), t)
            totals[0] += 1
            totals[1] += int(u)
            any_hit = False
            for s in range(129):
                if c[s] >= mk:
                    qh[s] += 1
                    kf[s] += int(c[s])
                    any_hit = True
            totals[3] += any_hit
        got = p.tally(t)
        assert np.array_equal(got[0], qh) and np.array_equal(got[1], kf) and np.array_equal(got[2], totals), t
    assert np.array_equal(p.tally(0.0)[0], np.full(129, 8, np.uint64))          # every sample is hit by every counted query
    both = T.add(p.tally(thr, slice(0, 4)), p.tally(thr, slice(4, None)))
    assert all(np.array_equal(a, b) for a, b in zip(both, p.tally(thr)))


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    L.bigsi_cpu_search_tally.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.bigsi_cpu_search_tally.restype = C.c_int32
    return L


def twin_index(L, p, h=T.H):
    from bigsi_amd._lib import Info
    ix = C.c_void_p()
    assert L.bigsi_cpu_open(C.c_uint64(T.M), C.c_uint64(p.n_cols), C.c_uint64(p.n_cols), C.c_uint32(h), 0, C.byref(ix)) == 0
    inf = Info()
    assert L.bigsi_cpu_get_info(ix, C.byref(inf)) == 0
    rows = p.junk_rows(int(inf.row_stride_bytes))
    ids = np.arange(T.M, dtype=np.uint64)
    assert L.bigsi_cpu_set_rows(ix, ptr(ids), C.c_uint64(T.M), ptr(rows), C.c_uint64(rows.shape[1])) == 0, L.bigsi_cpu_last_error()
    return ix


def twin_tally(L, ix, seqs, thr, n_cols, capacity=None):
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(seqs)
    qh, kf, totals = np.full(n_cols + 1, 0xAB, np.uint64), np.full(n_cols + 1, 0xAB, np.uint64), np.full(4, 0xAB, np.uint64)
    rc = L.bigsi_cpu_search_tally(ix, blob, ptr(off), len(seqs), T.K, thr, ptr(qh), ptr(kf), n_cols if capacity is None else capacity, ptr(totals))
    assert qh[n_cols] == 0xAB and kf[n_cols] == 0xAB
    return rc, qh[:n_cols], kf[:n_cols], totals


@pytest.mark.parametrize("n_cols", WIDTHS)
def test_twin_against_numpy(cpu, n_cols):
    p = T.planted(n_cols, 9)
    ix = twin_index(cpu, p)
    for thr in (1.0, p.edge_threshold()[0], 0.0, -1.0):
        rc, qh, kf, totals = twin_tally(cpu, ix, p.seqs, thr, n_cols)
        want = p.tally(thr)
        assert rc == 0, cpu.bigsi_cpu_last_error()
        assert np.array_equal(qh, want[0]) and np.array_equal(kf, want[1]) and np.array_equal(totals, want[2]), (n_cols, thr)
    assert cpu.bigsi_cpu_close(ix) == 0


def test_twin_refusals(cpu):
    p = T.planted(65, 9)
    ix = twin_index(cpu, p)
    rc, qh, kf, totals = twin_tally(cpu, ix, p.seqs, 1.0, 65, capacity=64)
    assert rc == ERR_CAPACITY and (qh == 0xAB).all() and (kf == 0xAB).all() and (totals == 0xAB).all()          # outputs untouched
    assert twin_tally(cpu, ix, p.seqs, 1.5, 65)[0] == ERR_INVALID and twin_tally(cpu, ix, p.seqs, float("nan"), 65)[0] == ERR_INVALID
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(p.seqs)
    out = np.zeros(65, np.uint64)
    tot = np.zeros(4, np.uint64)
    call = cpu.bigsi_cpu_search_tally
    for args in ((None, blob, ptr(off), 9, T.K, 1.0, ptr(out), ptr(out), 65, ptr(tot)), (ix, blob, None, 9, T.K, 1.0, ptr(out), ptr(out), 65, ptr(tot)),
                 (ix, blob, ptr(off), 9, T.K, 1.0, None, ptr(out), 65, ptr(tot)), (ix, blob, ptr(off), 9, T.K, 1.0, ptr(out), None, 65, ptr(tot)),
                 (ix, blob, ptr(off), 9, T.K, 1.0, ptr(out), ptr(out), 65, None), (ix, blob, ptr(off), 0, T.K, 1.0, ptr(out), ptr(out), 65, ptr(tot)),
                 (ix, blob, ptr(off), 9, 0, 1.0, ptr(out), ptr(out), 65, ptr(tot))):
        assert call(*args) == ERR_INVALID and cpu.bigsi_cpu_last_error()
    assert cpu.bigsi_cpu_close(ix) == 0
    empty = C.c_void_p()
    assert cpu.bigsi_cpu_open(C.c_uint64(64), C.c_uint64(0), C.c_uint64(8), C.c_uint32(3), 0, C.byref(empty)) == 0
    assert call(empty, blob, ptr(off), 9, T.K, 1.0, ptr(out), ptr(out), 65, ptr(tot)) == ERR_STATE
    assert cpu.bigsi_cpu_close(empty) == 0


# --------------------------------------------------------------------------------------------- the host layer
def test_order_ties_limit_and_deleted():
    from bigsi_amd import tally
    qh = np.array([3, 0, 7, 3, 7, 1, 3], np.uint64)
    kf = np.array([30, 0, 70, 31, 71, 10, 32], np.uint64)
    assert tally.order(qh).tolist() == [2, 4, 0, 3, 6, 5]                    # most queries first, ties to the lowest colour, zeros left out
    assert tally.order(qh, excluded=[4, 0]).tolist() == [2, 3, 6, 5] and tally.order(qh, excluded=np.array([9, 1], np.uint32)).tolist() == [2, 4, 0, 3, 6, 5]
    assert tally.order(np.zeros(5, np.uint64)).size == 0 and tally.order(np.array([1 << 63, (1 << 64) - 1], np.uint64)).tolist() == [1, 0]
    names = ["s%d" % c for c in range(7)]
    rows = tally.rows(qh, kf, names.__getitem__, excluded=[4])
    assert rows == [{"sample_name": "s2", "colour": 2, "queries_hit": 7, "kmers_found": 70}, {"sample_name": "s0", "colour": 0, "queries_hit": 3, "kmers_found": 30},
                    {"sample_name": "s3", "colour": 3, "queries_hit": 3, "kmers_found": 31}, {"sample_name": "s6", "colour": 6, "queries_hit": 3, "kmers_found": 32},
                    {"sample_name": "s5", "colour": 5, "queries_hit": 1, "kmers_found": 10}]
    assert all(type(v) is int for r in rows for k_, v in r.items() if k_ != "sample_name")
    assert tally.rows(qh, kf, names.__getitem__, excluded=[4], limit=2) == rows[:2] and tally.rows(qh, kf, names.__getitem__, excluded=[4], limit=99) == rows
    for bad, err in ((0, ValueError), (-1, ValueError), (True, TypeError), (2.0, TypeError), ("2", TypeError)):
        with pytest.raises(err):
            tally.rows(qh, kf, names.__getitem__, limit=bad)
    rec = tally.record(qh, kf, np.array([9, 400, 2, 8], np.uint64), names.__getitem__, excluded=[4], limit=3)
    assert list(rec) == ["queries", "kmers", "skipped", "queries_with_hits", "samples"]
    assert (rec["queries"], rec["kmers"], rec["skipped"], rec["queries_with_hits"]) == (9, 400, 2, 8) and rec["samples"] == rows[:3]


def test_json_and_csv_text():
    from bigsi_amd import tally
    qh, kf = np.array([2, 5, 0], np.uint64), np.array([20, 55, 0], np.uint64)
    names = ['plain', 'a,b "c"', "z"]
    rec = tally.record(qh, kf, [5, 60, 1, 5], names.__getitem__)
    assert json.loads(tally.to_json(rec)) == rec
    assert tally.to_json(rec) == ('{"queries": 5, "kmers": 60, "skipped": 1, "queries_with_hits": 5, "samples": [{"sample_name": "a,b \\"c\\"", "colour": 1, '
                                  '"queries_hit": 5, "kmers_found": 55}, {"sample_name": "plain", "colour": 0, "queries_hit": 2, "kmers_found": 20}]}')
    assert tally.to_csv(rec) == 'sample_name,colour,queries_hit,kmers_found\n"a,b ""c""",1,5,55\nplain,0,2,20'
    assert tally.to_csv(tally.record(np.zeros(3, np.uint64), kf, [0, 0, 4, 0], names.__getitem__)) == tally.CSV_HEADER


class _FakeIndex(object):
    def __init__(self):
        self.asked = None

    def tally(self, seqs, threshold=1.0, limit=None):
        self.asked = (list(seqs), threshold, limit)
        return {"queries": 2, "kmers": 9, "skipped": 0, "queries_with_hits": 1, "samples": [{"sample_name": "s", "colour": 4, "queries_hit": 1, "kmers_found": 5}]}


def test_cli_parsing_and_text(capsys):
    from bigsi_amd.__main__ import build_parser, main, tally_text
    p = build_parser()[0]
    a = p.parse_args(["tally", "reads.fasta", "-c", "c.yaml"])
    assert (a.cmd, a.fasta, a.threshold, a.limit, a.format, a.config) == ("tally", "reads.fasta", 1.0, None, "json", "c.yaml")
    a = p.parse_args(["tally", "reads.fasta", "-t", "0.4", "--limit", "7", "--format", "csv"])
    assert (a.threshold, a.limit, a.format) == (0.4, 7, "csv")
    for argv in (["tally"], ["tally", "r.fa", "--limit", "0"], ["tally", "r.fa", "--format", "xml"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    p.format_help()
    ix = _FakeIndex()
    assert json.loads(tally_text(ix, ["ACGT", "TTTT"], 0.5, 3))["samples"][0]["colour"] == 4 and ix.asked == (["ACGT", "TTTT"], 0.5, 3)
    assert tally_text(ix, ["ACGT"], fmt="csv") == "sample_name,colour,queries_hit,kmers_found\ns,4,1,5"
    with pytest.raises(SystemExit):
        main(["tally", "reads.fasta", "--sharded"])
    err = capsys.readouterr().err
    assert "--sharded" in err and "tally" in err


def test_tally_checks_its_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    for seqs, kw, err in (("ACGT", {}, TypeError), (b"ACGT", {}, TypeError), (["ACGT"], {"threshold": 1.5}, ValueError), (["ACGT"], {"threshold": float("nan")}, ValueError),
                          (["ACGT"], {"limit": 0}, ValueError)):
        with pytest.raises(err):
            b.tally(seqs, **kw)


def test_abi_lists_the_new_entry_points():
    from bigsi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_tally.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.TALLY_SIGNATURES) == ["bigsi_hip_tally_add_batch", "bigsi_hip_tally_add_stream", "bigsi_hip_tally_create", "bigsi_hip_tally_destroy",
                                                         "bigsi_hip_tally_fetch", "bigsi_hip_tally_reset"]
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.TALLY_SIGNATURES[name][1] and _lib.TALLY_SIGNATURES[name][0] is C.c_int
        assert all(name not in t for t in (_lib.SIGNATURES, _lib.COMPACT_SIGNATURES, _lib.FOLD_SIGNATURES, _lib.PREVALENCE_SIGNATURES, _lib.COLLAPSE_SIGNATURES,
                                           _lib.CONSENSUS_SIGNATURES, _lib.PAIRWISE_SIGNATURES))
        assert name not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip.h")).read(), flags=re.S)
    assert len(_lib.TALLY_SIGNATURES["bigsi_hip_tally_add_stream"][1]) == 6 and _lib.TALLY_SIGNATURES["bigsi_hip_tally_add_stream"][1][3] is C.c_uint64
    assert "bigsi_cpu_search_tally" in open(os.path.join(ROOT, "include", "bigsi_cpu_tally.h")).read()


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planners_and_twin(tmp_path):
    """tests/c_host/tally_sanitize_main.cpp -- a program with its own main that drives plan_tally, plan_tally_chunks and the twin's
    bigsi_cpu_search_tally over odd shapes -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its
    own."""
    exe = str(tmp_path / "tally_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "tally_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "tally planners and twin: ok", (r.stdout[-1000:], r.stderr[-3000:])
