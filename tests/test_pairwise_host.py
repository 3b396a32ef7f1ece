"""Pairwise popcounts without a GPU: the CPU twin of bigsi_hip_pairwise_popcounts against numpy on the very bits written
(expected = bits[:, A].T @ bits[:, B] in uint64), the invariants of plan_pairwise and the tables of pairwise_tables
(csrc/bigsi_launch.hpp, compiled by g++) -- and the three kernels' arithmetic replayed from them --, the arithmetic of
bigsi_amd/distances.py beside stats.derive_similar, what the argument checks refuse and in which order, the two command lines, and
a stand-alone sanitized program over the planner, the replay and the twin."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raw_index import ptr, ragged_bits

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
OK, ERR_INVALID, ERR_RANGE, ERR_CAPACITY = 0, -1, -4, -5
SENTINEL = 0xABABABABABABABAB
HEAD = ("total_words", "chunk_words", "chunks", "slice_words", "slices", "tiles_i", "tiles_j", "tiles", "plane_bytes", "partial_bytes")
CONSTS = ("max_pairs", "tile", "stage_words", "plane_bytes", "partial_bytes", "max_chunk_words", "split_words", "min_slice_words", "want_groups")


def expected(bits, a, b=None):
    b = a if b is None else b
    return bits[:, np.asarray(a, np.int64)].T.astype(np.uint64) @ bits[:, np.asarray(b, np.int64)].astype(np.uint64)


def selections(n, tile=64):
    """[(label, cols_a, cols_b or None)] for an index of n columns: one source word, the 63|64 straddle, first and last column,
    unsorted, repeats, overlapping lists, 1 x many and many x 1."""
    rng = np.random.default_rng(77 + n)
    every = np.arange(n, dtype=np.uint32)
    out = [("first_last", np.array([0, n - 1], np.uint32), None),
           ("one_word", every[:min(n, 64)][::3].copy(), None),
           ("unsorted", rng.permutation(n)[:min(n, tile + 1)].astype(np.uint32), None),
           ("repeats", np.array([n - 1, 0, n - 1, n // 2, 0, n - 1], np.uint32), None),
           ("overlap", every[:min(n, 40)].copy(), every[min(n, 40) // 2:min(n, 90)][::-1].copy()),
           ("one_by_many", np.array([n // 3], np.uint32), rng.permutation(n)[:min(n, 2 * tile + 1)].astype(np.uint32)),
           ("many_by_one", rng.permutation(n)[:min(n, 2 * tile + 1)].astype(np.uint32), np.array([n - 1], np.uint32))]
    if n > 64:
        out.append(("straddle", np.array([64, 63, 62, min(65, n - 1)], np.uint32), np.array([63, 64], np.uint32)))
    return out


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    L.bigsi_cpu_pairwise_popcounts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.bigsi_cpu_pairwise_popcounts.restype = C.c_int32
    return L


def twin_index(L, bits):
    m, n = bits.shape
    ix = C.c_void_p()
    assert L.bigsi_cpu_open(C.c_uint64(m), C.c_uint64(n), C.c_uint64(n), C.c_uint32(3), 0, C.byref(ix)) == 0
    packed = np.ascontiguousarray(np.packbits(bits, axis=1))
    ids = np.arange(m, dtype=np.uint64)
    assert L.bigsi_cpu_set_rows(ix, ptr(ids), C.c_uint64(m), ptr(packed), C.c_uint64(packed.shape[1])) == 0, L.bigsi_cpu_last_error()
    return ix


def twin_call(L, ix, a, b=None, capacity=None, out=None):
    na, nb = a.size, (a.size if b is None else b.size)
    if out is None:
        out = np.full((na, nb), SENTINEL, np.uint64)
    rc = L.bigsi_cpu_pairwise_popcounts(ix, ptr(a), na, ptr(b), 0 if b is None else nb, ptr(out), out.size if capacity is None else capacity)
    return rc, out


@pytest.mark.parametrize("n", (1, 65, 129, 1025))
def test_twin_against_numpy(cpu, n):
    bits = ragged_bits(131, n)
    ix = twin_index(cpu, bits)
    for label, a, b in selections(n):
        rc, out = twin_call(cpu, ix, a, b)
        assert rc == OK, (label, cpu.bigsi_cpu_last_error())
        assert np.array_equal(out, expected(bits, a, b)), label
    assert cpu.bigsi_cpu_close(ix) == 0


def test_twin_refusals_and_their_order(cpu):
    bits = ragged_bits(9, 70)
    ix = twin_index(cpu, bits)
    a, b = np.array([3, 69, 5], np.uint32), np.array([1, 2], np.uint32)
    bad = np.array([3, 70, 5], np.uint32)
    huge = np.zeros((1 << 14) + 1, np.uint32)          # (2^14 + 1)^2 pairs: above the cap
    out = np.full((3, 3), SENTINEL, np.uint64)
    for args, code, says in (((None, 3, None, 0, ptr(out), 9), ERR_INVALID, "NULL"),
                             ((ptr(a), 3, None, 0, None, 9), ERR_INVALID, "NULL"),
                             ((ptr(a), 0, None, 0, ptr(out), 9), ERR_INVALID, "empty"),
                             ((ptr(a), 3, ptr(b), 0, ptr(out), 9), ERR_INVALID, "empty"),
                             ((ptr(bad), 3, None, 0, ptr(out), 0), ERR_RANGE, "cols_a[1] = 70"),          # the entry is named before the capacity
                             ((ptr(a), 3, ptr(bad), 3, ptr(out), 0), ERR_RANGE, "cols_b[1] = 70"),
                             ((ptr(a), 3, None, 0, ptr(out), 8), ERR_CAPACITY, "capacity 8"),
                             ((ptr(a), 3, ptr(b), 2, ptr(out), 5), ERR_CAPACITY, "capacity 5"),
                             ((ptr(huge), huge.size, None, 0, ptr(out), 9), ERR_CAPACITY, "capacity 9"),  # the capacity before the cap
                             ((ptr(huge), huge.size, None, 0, ptr(out), 1 << 40), ERR_RANGE, "BIGSI_PAIRWISE_MAX_PAIRS")):
        assert cpu.bigsi_cpu_pairwise_popcounts(ix, *args) == code, (args, cpu.bigsi_cpu_last_error())
        assert says in cpu.bigsi_cpu_last_error().decode(), cpu.bigsi_cpu_last_error()
        assert (out == SENTINEL).all()
    assert cpu.bigsi_cpu_pairwise_popcounts(None, ptr(a), 3, None, 0, ptr(out), 9) == ERR_INVALID
    assert cpu.bigsi_cpu_close(ix) == 0
    header = open(os.path.join(ROOT, "include", "bigsi_hip_pairwise.h")).read()
    assert "#define BIGSI_PAIRWISE_MAX_PAIRS (1ull << 28)" in header


# --------------------------------------------------------------------------------------------- the planner and the tables
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pairwise_host") / "libpairwise_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "pairwise_host.cpp")])
    lib = C.CDLL(so)
    lib.pairwise_host_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.pairwise_host_chunk.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.pairwise_host_table_sizes.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.pairwise_host_replay.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


def constants(lib):
    c = np.zeros(9, np.uint64)
    lib.pairwise_host_constants(ptr(c))
    return dict(zip(CONSTS, (int(x) for x in c)))


def plan(lib, nua, nub, symmetric, m, stride_words=1 << 26):
    head = np.zeros(10, np.uint64)
    lib.pairwise_host_plan(nua, nub, int(symmetric), m, stride_words, ptr(head))
    return dict(zip(HEAD, (int(x) for x in head)))


def chunk(lib, nua, nub, symmetric, m, c, stride_words=1 << 26):
    w, s = C.c_uint64(0), C.c_uint64(0)
    lib.pairwise_host_chunk(nua, nub, int(symmetric), m, stride_words, c, C.byref(w), C.byref(s))
    return w.value, s.value


def test_plan_invariants(plan_lib):
    k = constants(plan_lib)
    assert k["max_pairs"] == 1 << 28 and k["tile"] == 64
    shapes = [(1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (129, 129), (1024, 1024), (4096, 4096), (16384, 16384), (1, 100_000), (100_000, 1), (64, 16384),
              (1, 1 << 28), (1 << 14, 1 << 14), (1 << 13, 1 << 14)]
    rows = [1, 63, 64, 65, 128, 129, 257, 1009, 2047, 2048, 2049, 4096, 70_001, 10_000_000, 1 << 33, (1 << 40) + 5]
    for nua, nub in shapes:
        for symmetric in (False, True):
            if symmetric and nua != nub:
                continue
            for m in rows:
                p = plan(plan_lib, nua, nub, symmetric, m)
                ctx = (nua, nub, symmetric, m, p)
                distinct = nua if symmetric else nua + nub
                assert p["total_words"] == -(-m // 64), ctx
                # the stated scratch cap, independent of the rows
                assert p["plane_bytes"] == distinct * p["chunk_words"] * 8 <= max(k["plane_bytes"], 16 * distinct), ctx
                assert p["partial_bytes"] == p["slices"] * 4 * nua * nub <= max(k["partial_bytes"], 4 * nua * nub), ctx
                # chunks and slices cover every 64-row word exactly once, none is empty
                assert 1 <= p["chunk_words"] <= k["max_chunk_words"] and (p["chunks"] - 1) * p["chunk_words"] < p["total_words"] <= p["chunks"] * p["chunk_words"], ctx
                covered = 0
                for c in sorted({0, 1, p["chunks"] // 2, p["chunks"] - 1}):
                    if c >= p["chunks"]:
                        continue
                    words, slices = chunk(plan_lib, nua, nub, symmetric, m, c)
                    assert words == min(p["chunk_words"], p["total_words"] - c * p["chunk_words"]) >= 1, ctx
                    assert 1 <= slices <= p["slices"] <= 65535 and (slices - 1) * p["slice_words"] < words <= slices * p["slice_words"], ctx
                    covered += words
                if p["chunks"] <= 3:
                    assert covered == p["total_words"], ctx
                # no 32-bit counter can wrap: a slice holds fewer than 2^32 rows
                assert p["slice_words"] * 64 < 1 << 32, ctx
                # tiles
                assert p["tiles_i"] == -(-nua // 64) and p["tiles_j"] == -(-nub // 64) and p["tiles"] == p["tiles_i"] * p["tiles_j"] < 1 << 31, ctx
                # two slices from 128 rows on (unless one slice's partials already fill the budget), three chunks from 2048 rows on
                if p["chunk_words"] >= 2 and 8 * nua * nub <= k["partial_bytes"]:
                    assert p["slices"] >= 2, ctx
                if p["total_words"] >= k["split_words"]:
                    assert p["chunks"] >= 3, ctx
                else:
                    assert p["chunks"] == 1 or p["plane_bytes"] >= k["plane_bytes"] // 2 or p["chunk_words"] == 2, ctx


def test_small_indexes_reach_the_sum_over_slices_and_chunks(plan_lib):
    """the sizes tests/test_gpu_pairwise.py uses"""
    for m in (257, 1009):
        p = plan(plan_lib, 5, 5, True, m, 16)
        assert p["chunks"] == 1 and p["slices"] >= 2
    for m in (2048, 4100, 70_001):
        p = plan(plan_lib, 5, 5, True, m, 16)
        assert p["chunks"] >= 3 and p["slices"] >= 2
    p = plan(plan_lib, 3, 3, True, 70_001, 16)
    assert p["chunks"] == 3 and p["slice_words"] * 64 < 70_001 / 3


@pytest.mark.parametrize("n", (65, 129, 8193))
def test_tables_and_kernel_arithmetic_replayed(plan_lib, n):
    """the three kernels' arithmetic, from the planner's tables, on the very bytes an index holds -- with rows behind num_rows that
    must not be counted"""
    for m, alloc in ((1, 1), (63, 64), (257, 300), (2049, 2049), (4100, 4100)):
        if n > 1000 and m > 300:
            continue
        bits = ragged_bits(alloc, n)
        stride = max(128, -(-n // 512) * 64)
        packed = np.zeros((alloc, stride), np.uint8)
        packed[:, :(n + 7) // 8] = np.packbits(bits, axis=1)
        for label, a, b in selections(n):
            sizes = np.zeros(4, np.uint64)
            plan_lib.pairwise_host_table_sizes(ptr(a), a.size, ptr(b), 0 if b is None else b.size, ptr(sizes))
            both = np.unique(a) if b is None else np.unique(np.concatenate([a, b]))
            assert [int(x) for x in sizes] == [both.size, np.unique(both // 64).size, np.unique(a).size, 0 if b is None else np.unique(b).size], label
            out = np.full((a.size, a.size if b is None else b.size), SENTINEL, np.uint64)
            rc = plan_lib.pairwise_host_replay(ptr(packed), m, stride, ptr(a), a.size, ptr(b), 0 if b is None else b.size, ptr(out))
            assert rc == 0, (label, m, rc)
            assert np.array_equal(out, expected(bits[:m], a, b)), (label, m)


# --------------------------------------------------------------------------------------------- distances.py
def test_derive_distances_is_derive_similar_row_by_row():
    from bigsi_amd.distances import derive_distances
    from bigsi_amd.stats import derive_similar
    rng = np.random.default_rng(5)
    bits = (rng.random((900, 12)) < rng.random(12)[None, :]).astype(np.uint8)
    bits[:, 4] = 0                                    # an empty filter: both denominators 0 against itself
    bits[:, 7] = bits[:, 2]                           # a duplicate: jaccard 1.0
    inter = expected(bits, np.arange(12))
    counts = bits.sum(axis=0).astype(np.uint64)
    assert np.array_equal(inter.diagonal(), counts)
    names = ["s%d" % c for c in range(12)]
    jac, con = derive_distances(inter, counts, counts)
    assert jac.dtype == con.dtype == np.float64 and jac[4, 4] == 0.0 and con[4, 3] == 0.0 and jac[2, 7] == 1.0
    for i in range(12):
        for r in derive_similar(counts, counts[i], inter[i], names, leave_out=i):
            c = r["colour"]
            assert (int(inter[i, c]), jac[i, c], con[i, c]) == (r["bits_shared"], r["jaccard"], r["containment"]), (i, c)
    assert np.array_equal(jac, jac.T)
    # rectangular: two own-count vectors
    j2, c2 = derive_distances(inter[:3, 5:], counts[:3], counts[5:])
    assert np.array_equal(j2, jac[:3, 5:]) and np.array_equal(c2, con[:3, 5:])
    with pytest.raises(ValueError):
        derive_distances(inter, counts[:3], counts)


def test_cluster_single_linkage_on_a_hand_made_matrix():
    from bigsi_amd.distances import cluster_single_linkage
    names = ["z", "b", "q", "a", "m", "k"]
    j = np.eye(6)
    for x, y, v in ((0, 3, 0.9), (3, 5, 0.8), (1, 4, 0.95), (2, 4, 0.49), (0, 1, 0.5 - 1e-12)):
        j[x, y] = j[y, x] = v
    want = {"z": ["z", "a", "k"], "b": ["b", "m"], "q": ["q"]}          # a chain joins z-a-k; groups by lowest member, under its name
    got = cluster_single_linkage(j, names, 0.5)
    assert got == want and list(got) == ["z", "b", "q"]
    assert cluster_single_linkage(j, names, 0.5) == got                  # deterministic
    upper = np.triu(j)                                                    # one triangle says as much
    assert cluster_single_linkage(upper, names, 0.5) == want
    assert cluster_single_linkage(j, names, 0.4999) == {"z": ["z", "b", "a", "m", "k"], "q": ["q"]}          # z-b at 0.5 - 1e-12 now joins the two
    assert cluster_single_linkage(j, names, 0.49) == {"z": names}
    assert cluster_single_linkage(j, names, 1.0) == {n: [n] for n in names}
    assert cluster_single_linkage(j, names, 1e-300) == {"z": names}                                           # (a jaccard of 0.0 never joins)
    assert cluster_single_linkage(np.eye(3), ["a", "b", "c"], 1e-300) == {"a": ["a"], "b": ["b"], "c": ["c"]}
    for bad in (0, 0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            cluster_single_linkage(j, names, bad)
    with pytest.raises(ValueError):
        cluster_single_linkage(j[:5], names, 0.5)
    with pytest.raises(ValueError):
        cluster_single_linkage(j, ["a"] * 6, 0.5)


def test_groups_tsv_round_trips_through_the_collapse_parser(tmp_path):
    from bigsi_amd.__main__ import collapse_groups
    from bigsi_amd.collapse import collapse_plan
    from bigsi_amd.distances import groups_to_tsv, to_matrix_csv
    groups = {"s0": ["s0", "s3", "s5"], "s1": ["s1"], "s2 x": ["s2 x", "s4"]}
    f = tmp_path / "g.tsv"
    f.write_text(groups_to_tsv(groups))
    pairs = collapse_groups(str(f))
    assert pairs == [(s, g) for g, members in groups.items() for s in members]
    names = ["s0", "s1", "s2 x", "s3", "s4", "s5"]
    group_of, out_names, members = collapse_plan(names, pairs)
    assert out_names == list(groups) and dict(zip(out_names, members)) == groups and group_of.tolist() == [0, 1, 2, 0, 2, 0]
    for bad in ({"g": ["a\tb"]}, {"g\n": ["a"]}, {"g": [" "]}):
        with pytest.raises(ValueError):
            groups_to_tsv(bad)
    assert to_matrix_csv(np.array([[1, 2], [3, 4]], np.uint64), ["a", "b"], ["x", "y,z"]) == ',x,"y,z"\na,1,2\nb,3,4'


# --------------------------------------------------------------------------------------------- decided before any device call
def test_python_refuses_before_any_device_call():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    for bad in (0, 0.0, -1, 1.5, "0.5", None, True, float("nan")):
        with pytest.raises(ValueError):
            b.cluster_samples(bad)
    names = ["s0", None, "s2"]
    assert b._selected_colours(None, names) == (["s0", "s2"], [0, 2])
    assert b._selected_colours(["s2", "s0", "s2"], names) == (["s2", "s0", "s2"], [2, 0, 2])
    for samples, err in (([], ValueError), (["s1"], KeyError), (["nope"], KeyError), ([None], KeyError), ("s0", TypeError)):
        with pytest.raises(err):
            b._selected_colours(samples, names)
    with pytest.raises(ValueError):
        b._selected_colours(None, [None, None])


def test_abi_lists_the_new_entry_points():
    from bigsi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_pairwise.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.PAIRWISE_SIGNATURES) == ["bigsi_hip_pairwise_phase_ms", "bigsi_hip_pairwise_popcounts"]
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.PAIRWISE_SIGNATURES[name][1]
        assert all(name not in t for t in (_lib.SIGNATURES, _lib.COMPACT_SIGNATURES, _lib.FOLD_SIGNATURES, _lib.PREVALENCE_SIGNATURES, _lib.COLLAPSE_SIGNATURES))
    header = open(os.path.join(ROOT, "include", "bigsi_cpu_pairwise.h")).read()
    assert "#define bigsi_hip_pairwise_popcounts bigsi_cpu_pairwise_popcounts" in header
    hip_h = open(os.path.join(ROOT, "include", "bigsi_hip.h")).read()
    assert "bigsi_hip_pairwise_popcounts" not in re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S)          # bigsi_hip.h keeps its entry points
    from bigsi_amd.distances import MAX_PAIRS
    assert MAX_PAIRS == 1 << 28


class _FakeIndex(object):
    def __init__(self):
        self.asked = []

    def sample_distances(self, samples=None, against=None):
        self.asked.append(("distances", samples, against))
        a = samples or ["s0", "s1"]
        b = against or a
        inter = np.arange(len(a) * len(b), dtype=np.uint64).reshape(len(a), len(b))
        return {"samples": a, "against": b, "bits_shared": inter, "jaccard": inter / 8.0, "containment": inter / 4.0}

    def cluster_samples(self, min_jaccard, samples=None):
        self.asked.append(("cluster", min_jaccard, samples))
        return {"s0": ["s0", "s2"], "s1": ["s1"]}


def test_cli_parsing_and_text(tmp_path, capsys):
    from bigsi_amd.__main__ import build_parser, cluster_text, collapse_groups, distances_text, main
    p = build_parser()[0]
    a = p.parse_args(["distances", "-s", "x", "-s", "y", "--against-file", "b.txt", "--format", "csv", "-c", "c.yaml"])
    assert (a.cmd, a.samples, a.samples_file, a.against_file, a.format, a.config) == ("distances", ["x", "y"], None, "b.txt", "csv", "c.yaml")
    a = p.parse_args(["cluster", "--min-jaccard", "0.9", "--samples-file", "s.txt", "--out", "g.tsv"])
    assert (a.cmd, a.min_jaccard, a.samples, a.samples_file, a.out) == ("cluster", 0.9, [], "s.txt", "g.tsv")
    with pytest.raises(SystemExit):
        p.parse_args(["cluster"])                     # --min-jaccard is required
    for argv in (["distances", "--sharded"], ["cluster", "--min-jaccard", "0.5", "--sharded"]):
        with pytest.raises(SystemExit):
            main(argv)
        err = capsys.readouterr().err
        assert "--sharded" in err and argv[0] in err
    ix = _FakeIndex()
    out = json.loads(distances_text(ix, ["a", "b"], ["c"]))
    assert out == {"samples": ["a", "b"], "against": ["c"], "bits_shared": [[0], [1]], "jaccard": [[0.0], [0.125]], "containment": [[0.0], [0.25]]}
    assert ix.asked[-1] == ("distances", ["a", "b"], ["c"])
    assert distances_text(ix, None, None, "csv") == "# bits_shared\n,s0,s1\ns0,0,1\ns1,2,3\n# jaccard\n,s0,s1\ns0,0.0,0.125\ns1,0.25,0.375\n# containment\n,s0,s1\ns0,0.0,0.25\ns1,0.5,0.75"
    f = tmp_path / "g.tsv"
    assert json.loads(cluster_text(ix, 0.5, None, str(f))) == {"s0": ["s0", "s2"], "s1": ["s1"]}
    assert collapse_groups(str(f)) == [("s0", "s0"), ("s2", "s0"), ("s1", "s1")] and ix.asked[-1] == ("cluster", 0.5, None)


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planner_replay_and_twin(tmp_path):
    """tests/c_host/pairwise_sanitize_main.cpp -- a program with its own main that drives plan_pairwise, pairwise_tables, the kernels'
    arithmetic replayed from them and the twin's bigsi_cpu_pairwise_popcounts over odd shapes -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a process of its own."""
    exe = str(tmp_path / "pairwise_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "pairwise_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "pairwise planner, replay and twin: ok", (r.stdout[-1000:], r.stderr[-3000:])
