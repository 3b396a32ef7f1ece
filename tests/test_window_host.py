"""Windowed search without a GPU: the CPU twin of bigsi_hip_window_search against the numpy reference of tests/window_ref.py on a
seeded bit matrix (row ids from the oracle's hashing, the expectation from the bytes written), the ABI of the new headers,
plan_window_search (csrc/bigsi_launch.hpp, compiled by g++), the host-only helpers of bigsi_amd/window.py over the twin's output, the
`window_search` command on a stubbed index, and a stand-alone sanitized program over the planner and the twin."""
import csv
import ctypes as C
import io
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raw_index import ptr, rand_seq
from oracle import coracle
from window_ref import RECORD_DTYPE, SENTINEL, Outputs, found_matrix, presence_from_rows, window_reference

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6


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
    assert hasattr(L, "bigsi_cpu_window_search"), "libbigsi_cpu.so has no bigsi_cpu_window_search"
    L.bigsi_cpu_window_search.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    return L


class Twin(object):
    """A twin index of m rows and n columns, every row written at the full stride with seeded random bytes (three quarters of the
    bits set): the pad behind column n - 1 holds junk."""

    def __init__(self, L, m, n, h, seed):
        self.L, self.ix, self.m, self.n, self.h = L, C.c_void_p(), m, n, h
        assert L.bigsi_cpu_open(C.c_uint64(m), C.c_uint64(n), C.c_uint64(n), C.c_uint32(h), 0, C.byref(self.ix)) == 0
        rng = np.random.default_rng(seed)
        stride = (n + 63) // 64 * 8
        self.rows = np.ascontiguousarray(rng.integers(0, 256, (m, stride), dtype=np.uint8) | rng.integers(0, 256, (m, stride), dtype=np.uint8))
        ids = np.arange(m, dtype=np.uint64)
        assert L.bigsi_cpu_set_rows(self.ix, ptr(ids), C.c_uint64(m), ptr(self.rows), C.c_uint64(stride)) == 0, L.bigsi_cpu_last_error()

    def want(self, seqs, k, window, threshold):
        return window_reference([presence_from_rows(self.rows, coracle.seq_rows(s, k, self.h, self.m), self.n) for s in seqs], window, threshold)

    def search(self, seqs, k, window, threshold, capacity, null=None):
        blob, off = pack(seqs)
        o = Outputs(len(seqs), capacity)
        args = {"used": ptr(o.used), "need": ptr(o.need), "off": ptr(o.off), "cols": ptr(o.cols), "recs": ptr(o.recs)}
        if null:
            args[null] = None
        rc = self.L.bigsi_cpu_window_search(self.ix, blob, ptr(off), len(seqs), k, window, threshold, args["used"], args["need"], args["off"], args["cols"],
                                            args["recs"], capacity)
        return rc, o

    def close(self):
        assert self.L.bigsi_cpu_close(self.ix) == 0


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.mark.parametrize("n,h", [(1, 1), (63, 3), (64, 2), (65, 3), (129, 9)])
def test_twin_against_numpy(cpu, n, h):
    rng = np.random.default_rng(7 * n + h)
    k = 7
    ix = Twin(cpu, 509, n, h, seed=n + h)
    a = rand_seq(rng, 60)
    seqs = [a + a[5:25] + a[:9], rand_seq(rng, k), rand_seq(rng, k - 1), "", rand_seq(rng, 23), "ACGTTGCA" * 6]
    try:
        hits = 0
        for window in (1, 2, 3, 15, 16, 17, 22, 200):
            for t in (1.0, 0.4, 0.75):
                want = ix.want(seqs, k, window, t)
                total = int(want[2][-1])
                rc, o = ix.search(seqs, k, window, t, total)
                assert rc == 0, cpu.bigsi_cpu_last_error()
                o.assert_equal(want)
                hits += total
                assert want[0].tolist() == [min(window, max(len(s) - k + 1, 0)) for s in seqs]
                assert want[1].tolist() == [math.ceil(w * t) for w in want[0].tolist()]
                if total:
                    rc, o = ix.search(seqs, k, window, t, total - 1)
                    assert rc == ERR_CAPACITY and np.array_equal(o.off[:len(seqs) + 1], want[2]) and np.array_equal(o.used[:len(seqs)], want[0])
                    assert np.array_equal(o.need[:len(seqs)], want[1]) and o.lists_untouched()
        assert hits > 0
    finally:
        ix.close()


def test_twin_refusals(cpu):
    ix = Twin(cpu, 509, 20, 2, seed=1)
    seqs = ["ACGTACGTTGCAAC", "ACG"]
    try:
        for window, t in ((0, 1.0), (65536, 1.0), (3, 0.0), (3, -0.5), (3, 1.0000001), (3, float("nan"))):
            rc, o = ix.search(seqs, 5, window, t, 100)
            assert rc == ERR_INVALID and (o.off == SENTINEL).all() and (o.used == SENTINEL).all() and o.lists_untouched(), (window, t)
        for null in ("used", "need", "off", "cols", "recs"):
            assert ix.search(seqs, 5, 3, 1.0, 100, null=null)[0] == ERR_INVALID, null
        assert ix.search(seqs, 0, 3, 1.0, 100)[0] == ERR_INVALID
        assert ix.search(seqs, 5, 65535, 1.0, 100)[0] == 0
    finally:
        ix.close()


def test_reference_on_a_hand_made_matrix():
    """The reference itself, on presence patterns small enough to read."""
    pres = np.zeros((10, 3), bool)
    pres[[1, 2, 3, 7, 8, 9], 0] = True          # two islands of three
    pres[:, 1] = True
    used, need, off, cols, recs = window_reference([pres, np.zeros((0, 3), bool)], 3, 1.0)
    assert used.tolist() == [3, 0] and need.tolist() == [3, 0] and off.tolist() == [0, 2, 2] and cols.tolist() == [0, 1]
    assert recs[0].tolist() == (3, 1, 1, 7, 2, 0) and recs[1].tolist() == (3, 0, 0, 7, 8, 0)
    used, need, _, cols, recs = window_reference([pres], 4, 0.5)
    assert need.tolist() == [2] and recs[0].tolist() == (3, 0, 0, 6, 5, 0)          # starts 0..2 and 5..6 hold >= 2; starts 3 and 4 hold 1
    assert found_matrix(pres, 4)[1][:, 0].tolist() == [3, 3, 2, 1, 1, 2, 3]
    used, need, off, _, recs = window_reference([pres], 50, 0.6)                      # clamped: one window of 10 positions
    assert used.tolist() == [10] and need.tolist() == [6] and recs["best_found"].tolist() == [6, 10] and recs["windows_passing"].tolist() == [1, 1]


# --------------------------------------------------------------------------------------------- the ABI
def header_names(name, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % prefix, src)))


def test_abi_of_the_new_headers(tmp_path):
    from bigsi_amd import _lib
    new = ["bigsi_hip_batch_window_search", "bigsi_hip_window_search"]
    assert header_names("bigsi_hip_window.h", "bigsi_hip_") == sorted(_lib.WINDOW_SIGNATURES) == new
    for name in new:
        assert name not in _lib.SIGNATURES and name not in _lib.PREVALENCE_SIGNATURES
    for other in ("bigsi_hip.h", "bigsi_hip_prevalence.h", "bigsi_hip_group.h", "bigsi_hip_testing.h", "bigsi_hip_text.h", "bigsi_hip_tally.h"):
        assert not set(new) & set(header_names(other, "bigsi_hip_")), other
    assert "bigsi_hip_window_set_limits" in header_names("bigsi_hip_testing.h", "bigsi_hip_")
    assert _lib.SIGNATURES["bigsi_hip_window_set_limits"][1] == [C.c_void_p, C.c_uint64, C.c_uint64]
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)      # noqa: E731
    decl = lambda src, prefix: {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\b%s(\w+)\s*\(([^;{]*?)\)\s*;" % prefix, src)}      # noqa: E731
    cpu_h, hip_h = open(os.path.join(ROOT, "include", "bigsi_cpu_window.h")).read(), open(os.path.join(ROOT, "include", "bigsi_hip_window.h")).read()
    c, h = decl(strip(cpu_h), "bigsi_cpu_"), decl(strip(hip_h), "bigsi_hip_")
    for name in new:
        assert len(h[name[len("bigsi_hip_"):]].split(",")) == len(_lib.WINDOW_SIGNATURES[name][1])
    assert sorted(c) == ["window_search"] and sorted(h) == ["batch_window_search", "window_search"]
    assert c["window_search"].replace("bigsi_cpu_index", "bigsi_hip_index") == h["window_search"]
    assert "#define bigsi_hip_window_search bigsi_cpu_window_search" in cpu_h and "BIGSI_USE_CPU_TWIN" in cpu_h
    assert hasattr(C.CDLL(LIB), "bigsi_cpu_window_search")
    assert np.dtype(RECORD_DTYPE).itemsize == 24
    from bigsi_amd.window import RECORD_DTYPE as product_dtype, WINDOW_MAX
    assert product_dtype == RECORD_DTYPE and WINDOW_MAX == 65535 and "#define BIGSI_WINDOW_MAX 65535u" in hip_h
    fields = re.search(r"typedef struct \{(.*?)\} bigsi_hip_window_hit;", strip(hip_h), flags=re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", fields) == list(RECORD_DTYPE.names)
    # the layer list of the core header names the new one; both headers are C99
    assert "bigsi_hip_window.h" in open(os.path.join(ROOT, "include", "bigsi_hip.h")).read()
    for hdr in ("bigsi_hip_window.h", "bigsi_cpu_window.h"):
        src = tmp_path / ("use_%s.c" % hdr[:-2])
        src.write_text('#include "%s"\nint main(void) { return bigsi_hip_window_search(0, 0, 0, 1, 3, 1, 1.0, 0, 0, 0, 0, 0, 0) == BIGSI_OK && sizeof(bigsi_hip_window_hit) == 24; }\n' % hdr)
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_binds_the_new_symbols():
    """The device library exports what the header declares, with the binding's argument types (loading it needs no GPU)."""
    from bigsi_amd import _lib
    for name, (res, args) in _lib.WINDOW_SIGNATURES.items():
        fn = getattr(_lib.lib(), name)
        assert fn.argtypes == args and fn.restype == res
    assert _lib.lib().bigsi_hip_window_set_limits.argtypes == [C.c_void_p, C.c_uint64, C.c_uint64]


# --------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("window_host") / "libwindow_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "window_host.cpp")])
    return C.CDLL(so)


PLAN_KEYS = ("max_we", "planes", "seg_starts", "tiles", "n_segs", "waves", "grid", "wvp", "partial_bytes", "steps_per_iter", "grid_too_large",
             "partial_too_large", "target", "cap", "window_max")


def plan(lib, n, window, wv, h, forced=0, cap=0, max_segs=1 << 16):
    n = np.asarray(n, np.uint32)
    out, segs, seg_off = np.zeros(15, np.uint64), np.zeros((max_segs, 4), np.uint32), np.zeros(n.size + 1, np.uint64)
    lib.window_host_plan(ptr(n), C.c_uint32(n.size), C.c_uint32(window), C.c_uint64(wv), C.c_uint32(h), C.c_uint64(forced), C.c_uint64(cap), ptr(out),
                         ptr(segs), C.c_uint64(max_segs), ptr(seg_off))
    p = dict(zip(PLAN_KEYS, (int(x) for x in out)))
    p["segs"], p["seg_off"] = segs[:min(p["n_segs"], max_segs)], seg_off
    return p


def check_plan(p, n, window, wv, h, forced=0, cap=0):
    assert p["target"] == 4096 and p["cap"] == 2 << 30 and p["window_max"] == 65535
    we = [min(x, window) for x in n]
    max_we = max(we, default=0)
    assert p["max_we"] == max_we
    # the plane bucket holds every count up to the largest window
    assert p["planes"] in (4, 8, 12, 16) and p["planes"] >= max(max_we.bit_length(), 1) and (1 << p["planes"]) - 1 >= max_we
    assert p["planes"] == max(-(-max_we.bit_length() // 4) * 4, 4)
    # the segments tile [0, n - We] of every sequence exactly: no start twice, none missing, each at most S long
    assert p["seg_off"][0] == 0 and p["seg_off"][-1] == p["n_segs"]
    if p["n_segs"] <= len(p["segs"]):
        for q, x in enumerate(n):
            mine = p["segs"][int(p["seg_off"][q]):int(p["seg_off"][q + 1])]
            nxt = 0
            for sq, a, b, w in mine.tolist():
                assert sq == q and w == we[q] and a == nxt and a < b and b - a <= p["seg_starts"]
                nxt = b
            assert nxt == (x - we[q] + 1 if we[q] else 0)
            if we[q]:
                assert len(mine) == -(-(x - we[q] + 1) // p["seg_starts"])
    # S: forced, or between max(We, 64) and max(4 We, 64), shorter than 4 We only to reach the wavefront target
    if max_we:
        starts = sum(x - w + 1 for x, w in zip(n, we) if w)
        if forced:
            assert p["seg_starts"] == forced
        else:
            lo, hi = max(max_we, 64), max(4 * max_we, 64)
            assert lo <= p["seg_starts"] <= hi
            if p["seg_starts"] < hi:
                assert -(-starts // p["seg_starts"]) * p["tiles"] <= p["target"] + len(n) * p["tiles"] or p["seg_starts"] == lo
    # sizes, exactly
    assert p["tiles"] == max(-(-wv // 128), 1) and p["wvp"] == (wv + 1) // 2 * 2
    assert p["waves"] == p["n_segs"] * p["tiles"] and p["grid"] == -(-p["waves"] // 4)
    assert p["partial_bytes"] == p["n_segs"] * p["planes"] * p["wvp"] * 8
    assert p["steps_per_iter"] == (4 if h <= 1 else 2 if h <= 3 else 1) and 2 * min(h, 7) * p["steps_per_iter"] <= 14
    assert p["grid_too_large"] == int(p["grid"] > 0x7FFFFFFF)
    assert p["partial_too_large"] == int(p["partial_bytes"] > (cap or 2 << 30))


def test_plan_pinned_shapes(plan_lib):
    # one 100 kbp query, W = 1000, on 100 k samples (1563 words, 13 tiles): S stays at its floor, the window; 100 segments
    n = [100000 - 30]
    p = plan(plan_lib, n, 1000, 1563, 4)
    check_plan(p, n, 1000, 1563, 4)
    assert (p["planes"], p["seg_starts"], p["n_segs"], p["tiles"], p["waves"], p["grid"]) == (12, 1000, 99, 13, 1287, 322)
    assert p["partial_bytes"] == 99 * 12 * 1564 * 8
    # many 1 kbp queries: enough wavefronts, S = 4 We
    n = [970] * 4096
    p = plan(plan_lib, n, 100, 1563, 3)
    check_plan(p, n, 100, 1563, 3)
    assert (p["planes"], p["seg_starts"], p["n_segs"]) == (8, 400, 3 * 4096)
    # the plane buckets at their edges: We = 2^P - 1 and 2^P
    for we, planes in ((1, 4), (15, 4), (16, 8), (255, 8), (256, 12), (4095, 12), (4096, 16), (65535, 16)):
        p = plan(plan_lib, [we + 10], we, 3, 3)
        check_plan(p, [we + 10], we, 3, 3)
        assert p["planes"] == planes and plan_lib.window_host_bucket(we) == planes and plan_lib.window_host_bit_width(we) == we.bit_length()
    # the window clamped by a short sequence decides the bucket, not the window asked for
    p = plan(plan_lib, [12, 0, 3], 60000, 3, 3)
    check_plan(p, [12, 0, 3], 60000, 3, 3)
    assert (p["max_we"], p["planes"], p["n_segs"]) == (12, 4, 2) and p["segs"].tolist() == [[0, 0, 1, 12], [2, 0, 1, 3]]
    # nothing to sweep
    for n in ([], [0, 0]):
        p = plan(plan_lib, n, 5, 1563, 4)
        check_plan(p, n, 5, 1563, 4)
        assert p["n_segs"] == 0 and p["grid"] == 0 and p["partial_bytes"] == 0 and not p["grid_too_large"] and not p["partial_too_large"]
    # forced segments of 64 starts
    p = plan(plan_lib, [3000], 100, 3, 3, forced=64)
    check_plan(p, [3000], 100, 3, 3, forced=64)
    assert p["seg_starts"] == 64 and p["n_segs"] == -(-2901 // 64)


def test_plan_refusals(plan_lib):
    # the partial cap: the default 2 GiB, and a forced one
    n = [65535 * 2] * 12000
    p = plan(plan_lib, n, 65535, 1563, 4, max_segs=1)
    assert p["partial_bytes"] == p["n_segs"] * 16 * 1564 * 8 > 2 << 30 and p["partial_too_large"] == 1 and not p["grid_too_large"]
    p = plan(plan_lib, [3000], 100, 3, 3, forced=64, cap=1024)
    assert p["partial_bytes"] == 46 * 8 * 4 * 8 > 1024 and p["partial_too_large"] == 1
    assert plan(plan_lib, [3000], 100, 3, 3, forced=64, cap=46 * 8 * 4 * 8)["partial_too_large"] == 0
    # the grid: 2^31 - 1 workgroups
    n = [1 << 22] * 64
    p = plan(plan_lib, n, 1, 1 << 20, 1, forced=1, cap=1 << 62, max_segs=1)
    assert p["n_segs"] == 64 << 22 and p["grid"] == (64 << 22) * (1 << 13) // 4 > 0x7FFFFFFF and p["grid_too_large"] == 1


def test_plan_invariants_over_seeded_shapes(plan_lib):
    rng = np.random.default_rng(5)
    for _ in range(1500):
        n = [int(rng.choice([0, 1, 2, 15, 16, 17, 255, 256, 257, 970, 3000, int(rng.integers(1, 20000))])) for _ in range(int(rng.integers(1, 6)))]
        window = int(rng.choice([1, 2, 3, 15, 16, 255, 256, 1000, 4095, 4096, 65535, int(rng.integers(1, 65536))]))
        wv = int(rng.choice([1, 2, 3, 127, 128, 129, 157, 1563]))
        h = int(rng.integers(1, 12))
        forced = int(rng.choice([0, 0, 1, 64, 1000]))
        cap = int(rng.choice([0, 0, 4096, 1 << 20]))
        check_plan(plan(plan_lib, n, window, wv, h, forced, cap), n, window, wv, h, forced, cap)


# --------------------------------------------------------------------------------------------- bigsi_amd/window.py over the twin
def test_python_layer_over_the_twin(cpu):
    from bigsi_amd.window import RESULT_KEYS, assemble, check_args, to_csv, to_json, window_need
    rng = np.random.default_rng(3)
    k, window, t = 7, 10, 0.7
    ix = Twin(cpu, 509, 12, 2, seed=9)
    seqs = [rand_seq(rng, 60), "ACG", rand_seq(rng, 14)]
    try:
        want = ix.want(seqs, k, window, t)
        total = int(want[2][-1])
        rc, o = ix.search(seqs, k, window, t, total)
        assert rc == 0 and total > 4
        names = ["s%d" % c for c in range(12)]
        recs = assemble(seqs, k, window, t, o.used, o.need, o.off, o.cols, o.recs, lambda c: names[c], excluded=[])
        assert [tuple(r) for r in recs] == [("num_kmers", "window", "min_found", "results")] * 3
        assert recs[1] == {"num_kmers": 0, "window": 0, "min_found": 0, "results": []}
        assert (recs[0]["num_kmers"], recs[0]["window"], recs[0]["min_found"]) == (54, 10, 7) and (recs[2]["num_kmers"], recs[2]["window"], recs[2]["min_found"]) == (8, 8, 6)
        for i, rec in enumerate(recs):
            lo, hi = int(want[2][i]), int(want[2][i + 1])
            assert len(rec["results"]) == hi - lo
            # order: best_found descending, ties to the lowest colour
            keys = [(-r["best_found"], r["colour"]) for r in rec["results"]]
            assert keys == sorted(keys)
            by_colour = {int(c): want[4][lo + j] for j, c in enumerate(want[3][lo:hi])}
            for r in rec["results"]:
                assert tuple(r) == RESULT_KEYS and all(type(r[key]) is int for key in RESULT_KEYS if key not in ("sample_name", "percent_found"))
                w = by_colour[r["colour"]]
                assert r["sample_name"] == names[r["colour"]] and r["best_found"] == int(w["best_found"]) and r["best_start"] == int(w["best_start"])
                # coordinates: 0-based bases, [first_start, last_start + We + k - 1)
                assert r["match_start"] == int(w["first_start"]) and r["match_end"] == int(w["last_start"]) + rec["window"] + k - 1 <= len(seqs[i])
                assert r["windows_passing"] == int(w["windows_passing"]) and r["percent_found"] == 100.0 * r["best_found"] / rec["window"]
        assert len({r["best_found"] for r in recs[0]["results"]}) < len(recs[0]["results"])          # (there are ties to order)
        # a deleted sample is dropped
        gone = recs[0]["results"][0]["colour"]
        less = assemble(seqs, k, window, t, o.used, o.need, o.off, o.cols, o.recs, lambda c: names[c], excluded=np.asarray([gone], np.uint32))
        assert [r for r in recs[0]["results"] if r["colour"] != gone] == less[0]["results"] and len(less[0]["results"]) == len(recs[0]["results"]) - 1
        # the device's window and need are checked against the host's
        bad = o.need.copy()
        bad[0] += 1
        with pytest.raises(ValueError):
            assemble(seqs, k, window, t, o.used, bad, o.off, o.cols, o.recs, lambda c: names[c])
        # text
        got = json.loads(to_json(recs, seqs))
        assert [list(g)[0] for g in got] == ["query"] * 3 and got[0]["query"] == seqs[0] and got[0]["results"] == recs[0]["results"]
        rows = list(csv.reader(io.StringIO(to_csv(recs))))
        assert rows[0] == ["record"] + list(RESULT_KEYS) and len(rows) == 1 + total
        first = recs[0]["results"][0]
        assert rows[1] == ["0"] + [str(first[key]) for key in RESULT_KEYS] and rows[-1][0] == "2"
    finally:
        ix.close()
    # refusals mirror the C ABI
    assert check_args(1, 1) == (1, 1.0) and check_args(65535, 0.5) == (65535, 0.5) and window_need(8, 10, 0.7) == (8, 6) and window_need(0, 10, 0.7) == (0, 0)
    for window, t in ((0, 1.0), (65536, 1.0), (-1, 1.0), (5, 0.0), (5, 1.01), (5, -1), (5, float("nan"))):
        with pytest.raises(ValueError):
            check_args(window, t)
    for window in (1.5, "3", True, None):
        with pytest.raises(TypeError):
            check_args(window, 1.0)


class StubIndex(object):
    kmer_size = 3

    def __init__(self):
        self.calls = []

    def search_windows(self, seq, window, threshold=1.0):
        self.calls.append((seq, window, threshold))
        n = max(len(seq) - 2, 0)
        res = [{"sample_name": "a,b", "colour": 4, "best_found": 2, "percent_found": 100.0, "best_start": 1, "match_start": 1, "match_end": 6, "windows_passing": 1}] if n else []
        return {"num_kmers": n, "window": min(n, window), "min_found": min(n, window), "results": res}


def test_cli_parsing_and_text(tmp_path, capsys):
    import bigsi_amd.__main__ as cli
    p = cli.build_parser()[0]
    a = p.parse_args(["window_search", "ACGT", "--window", "5", "-t", "0.8", "--format", "csv", "--config", "c.yaml"])
    assert (a.cmd, a.seq, a.fasta, a.window, a.threshold, a.format) == ("window_search", "ACGT", None, 5, 0.8, "csv")
    a = p.parse_args(["window_search", "--fasta", "q.fa", "--window", "9", "--config", "c.yaml"])
    assert (a.seq, a.fasta, a.window, a.threshold, a.format) == (None, "q.fa", 9, 1.0, "json")
    ix = StubIndex()
    got = json.loads(cli.window_search_text(ix, ["ACGTA", "AC"], 2, 0.9, "json"))
    assert ix.calls == [("ACGTA", 2, 0.9), ("AC", 2, 0.9)]
    assert [list(g) for g in got] == [["query", "num_kmers", "window", "min_found", "results"]] * 2 and got[0]["query"] == "ACGTA" and got[1]["results"] == []
    assert got[0]["results"][0]["match_end"] == 6
    text = cli.window_search_text(ix, ["ACGTA", "AC", "GGGG"], 2, 1.0, "csv")
    assert text.split("\n") == ["record,sample_name,colour,best_found,percent_found,best_start,match_start,match_end,windows_passing",
                                '0,"a,b",4,2,100.0,1,1,6,1', '2,"a,b",4,2,100.0,1,1,6,1']
    cf = tmp_path / "c.yaml"
    cf.write_text("k: 3\nm: 100\nh: 2\nstorage-engine: hip-hbm\nstorage-config: {name: never-opened}\n")
    for argv, word in ((["window_search", "ACGT", "--window", "3", "--sharded", "--config", str(cf)], "--sharded"),
                       (["window_search", "--window", "3", "--config", str(cf)], "SEQ or --fasta"),
                       (["window_search", "ACGT", "--fasta", "q.fa", "--window", "3", "--config", str(cf)], "SEQ or --fasta"),
                       (["window_search", "ACGT", "--window", "0", "--config", str(cf)], "window must be"),
                       (["window_search", "ACGT", "--window", "70000", "--config", str(cf)], "window must be"),
                       (["window_search", "ACGT", "--window", "3", "-t", "0", "--config", str(cf)], "threshold must be"),
                       (["window_search", "ACGT", "--config", str(cf)], "--window")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_group_indexes_and_bad_arguments_are_refused():
    """devices=[...] indexes: refused in Python before the device is asked; so are the arguments the C ABI refuses."""
    from bigsi_amd._lib import ERR_STATE, BigsiHipError
    from bigsi_amd.graph.bigsi import BIGSI
    from bigsi_amd.storage.hip_hbm import HipHbmStorage

    def fresh(group):
        o = BIGSI.__new__(BIGSI)
        o.storage = HipHbmStorage.__new__(HipHbmStorage)
        o.storage.res = type("R", (), {"is_group": group})()
        return o
    for call in (lambda o: o.search_windows_many(["ACGT"], 3), lambda o: o.search_windows("ACGT", 3), lambda o: o.storage.window_search(["ACGT"], 3, 3)):
        with pytest.raises(BigsiHipError) as e:
            call(fresh(True))
        assert e.value.code == ERR_STATE and "multi-GPU" in str(e.value)
    for args in ((["ACGéT"], 3), (["ACGT"], 0), (["ACGT"], 65536), (["ACGT"], 3, 0.0), (["ACGT"], 3, 1.5)):
        with pytest.raises(ValueError):
            fresh(False).search_windows_many(*args)
    with pytest.raises(TypeError):
        fresh(False).search_windows_many("ACGT", 3)


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planner_and_twin(tmp_path):
    """tests/c_host/window_sanitize_main.cpp -- a program with its own main that drives plan_window_search and the twin's
    bigsi_cpu_window_search over the edge shapes -- built with AddressSanitizer and UBSan and run as a program: it must end clean."""
    exe = str(tmp_path / "window_sanitize")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "window_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "window planner and twin: ok" and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
