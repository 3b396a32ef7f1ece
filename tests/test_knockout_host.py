"""CPU-only: the knock-out index of the exact-search tests (tests/knockout_cases.py) held to what it promises, before the device
sees it: (1) coverage -- every segment that is wide enough knocks every row of R, every segment knocks the head of `order`, and the
telling list positions stand in that head; (2) sensitivity by mutation in numpy -- one row reference taken out of a query's list
changes that query's exact answer, for sampled queries and sampled references of every case; (3) the batch reference (one matrix
product) equals the per-sequence reference; (4) every case's route, against the compiled planner (tests/c_host/launch_host.cpp,
band_plan_host.cpp): a case that moves off the route it is built for fails here; (5) the ABI of the two read-only test entry points
(bigsi_hip_batch_last_row_and, bigsi_hip_batch_fetch_rows_sorted) without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import knockout_cases as kc
from conftest import ROOT
from knockout_cases import CASES, K, build_case, references

NAMES = [c["name"] for c in CASES]


def _build(tmp, name):
    so = str(tmp / ("lib%s.so" % name))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "c_host", name + ".cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("knockout_host")
    L, B = _build(tmp, "launch_host"), _build(tmp, "band_plan_host")
    L.launch_host_plan.restype = C.c_uint64
    L.launch_host_sort_rows_block.restype = C.c_uint32
    L.launch_host_sort_rows_block.argtypes = [C.c_uint64, C.c_uint32]
    B.band_host_plan.restype = C.c_uint64
    B.band_host_sort_shift.restype = C.c_uint32
    B.band_host_sort_shift.argtypes = [C.c_uint64, C.c_uint64]
    return L, B


def row_and_plan(L, n_seqs, wv, max_pos, h, early):
    head, launches = np.zeros(11, np.uint64), np.zeros(8 * 64, np.uint64)
    n = L.launch_host_plan(C.c_uint32(n_seqs), C.c_uint64(wv), C.c_uint64(max_pos), C.c_uint32(h), 1, 0, int(early), 0,
                           head.ctypes.data_as(C.c_void_p), launches.ctypes.data_as(C.c_void_p), C.c_uint64(64))
    keys = ("too_large", "slices", "want_sorted", "preset", "P", "count_bytes", "planes_out", "combine", "deep", "early", "n_launches")
    lk = ("q0", "q1", "grid", "block", "tiles", "slices", "unroll", "needs_preset")
    return dict(zip(keys, head.tolist())), [dict(zip(lk, launches[8 * i:8 * i + 8].tolist())) for i in range(int(n))]


def k1_plan(L, n_seqs, max_pos, max_len, force_global):
    out = np.zeros(6, np.uint64)
    L.launch_host_k1_plan(C.c_uint32(n_seqs), C.c_uint64(max_pos), C.c_uint64(max_len), 0, int(force_global), out.ctypes.data_as(C.c_void_p))
    return dict(zip(("route", "hs_cap", "sq_bytes", "tab_mult", "tab_cap", "lds"), out.tolist()))


def band_plan(B, n_seqs, wv, max_pos, h, m, forced, windows, segs):
    head, launches = np.zeros(9, np.uint64), np.zeros(5, np.uint64)
    B.band_host_plan(C.c_uint32(n_seqs), C.c_uint64(wv), C.c_uint64(max_pos), C.c_uint32(h), 1, 0, 0, C.c_uint64(m), int(forced),
                     C.c_uint32(windows), C.c_uint32(segs), head.ctypes.data_as(C.c_void_p), launches.ctypes.data_as(C.c_void_p), C.c_uint64(1))
    return dict(zip(("taken", "windows", "segs_per_launch", "seg_groups", "unroll", "grid", "in_flight", "n_launches", "merge_tail"), head.tolist()))


# --------------------------------------------------------------------------------------------- (1) coverage
@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_knocked_where_the_segment_is_wide_enough(name):
    c, ko, queries = build_case(name)
    assert queries[0] == ko.main and ko.r == np.unique(ko.hash_list).size and ko.hash_list.size == ko.u * c["h"]
    assert np.array_equal(np.sort(ko.order), np.arange(ko.r))
    # the telling positions are the head of `order`, in the order they were named
    named = [j for _, j in ko.named]
    assert ko.order[:ko.n_head].tolist() == [j for i, j in enumerate(named) if j not in named[:i]]
    what = " ".join(w for w, _ in ko.named)
    for key in ("hash[0] first", "addr[0] first", "last", "tail of unroll 8", "tail of unroll 4", "tail of unroll 2"):
        assert key in what, key
    for S in c.get("slices", ()):
        assert "first of slice %d of %d" % (min(S - 1, -(-ko.hash_list.size // -(-ko.hash_list.size // S)) - 1), S) in what
    for W, _ in c.get("windows", ()):
        assert W == 1 or "first of window %d of %d" % (min(W, 64) - 1, W) in what
    n_segs = -(-c["n_cols"] // kc.SEG_COLS)
    some_full = False
    for s in range(n_segs):
        lo, hi = s * kc.SEG_COLS, min((s + 1) * kc.SEG_COLS, c["n_cols"])
        got = set(ko.knocked[lo:hi][ko.knocked[lo:hi] >= 0].tolist())
        if s == c.get("tenth_segment"):
            # none FULL, and only rows of the first tenth of the address order
            assert (ko.knocked[lo:hi] >= 0).all() and max(got) < max(ko.r // 10, 1)
            continue
        if ko.covered[s]:
            assert got == set(range(ko.r)), (name, s)
            some_full = True
        else:
            # the stated exception: a segment narrower than r knocks the head of `order`, at least the telling positions when it
            # has the columns for them
            assert got == set(ko.order[:ko.seg_cover[s]].tolist()), (name, s)
            assert ko.seg_cover[s] >= min(ko.n_head, hi - lo - 6), (name, s)
        # the named edge columns are FULL
        for col in (lo, lo + 63, lo + 64, lo + 127, hi - 1):
            assert col >= hi or ko.knocked[col] < 0, (name, col)
    assert some_full or c["kind"] == "reads", "no segment of the case knocks every row"
    # the index is what the text says: a FULL column has every row, a knock-out every row but its own
    zeros = np.argwhere(~ko.bits)
    assert np.array_equal(zeros[:, 0], ko.knocked[zeros[:, 1]]) and zeros.shape[0] == np.count_nonzero(ko.knocked >= 0)
    assert np.array_equal(np.unpackbits(ko.packed, axis=1)[:, :c["n_cols"]].astype(bool), ko.bits)


# --------------------------------------------------------------------------------------------- (2) sensitivity
def sampled_queries(n, rng):
    return list(range(n)) if n <= 48 else sorted(set(range(12)) | set(rng.choice(n, size=36, replace=False).tolist()))


@pytest.mark.parametrize("name", NAMES)
def test_a_single_removed_row_reference_changes_the_answer(name):
    """For sampled queries: the exact answer (AND over the rows the query references, as written; an unwritten row is zero), then
    with ONE reference taken out -- first, last and three sampled positions of the query's list.  A reference whose row the list
    holds twice is legitimate to skip and not sampled; in a case whose segments are all narrower than r (the read cases at h = 4)
    only references to rows some column knocks are sampled."""
    c, ko, queries = build_case(name)
    rng = np.random.default_rng(5)
    everywhere = bool(ko.covered.any())
    knocked_rows = ko.R[np.unique(ko.knocked[ko.knocked >= 0])]
    tried = 0
    for qi in sampled_queries(len(queries), rng):
        first, _ = kc.coracle.unique_kmers(queries[qi], K)
        if len(first) == 0:
            continue
        lst = kc.coracle.seq_rows(queries[qi], K, c["h"], c["m"])[first].astype(np.uint64).ravel()
        rows, mult = np.unique(lst, return_counts=True)
        idx = np.minimum(np.searchsorted(ko.row_ids, rows), ko.row_ids.size - 1)
        assert (ko.row_ids[idx] == rows).all()
        zeros = (~ko.bits[idx]).sum(axis=0)
        single = rows[mult == 1] if everywhere else np.intersect1d(rows[mult == 1], knocked_rows)
        cand = [p for p in range(lst.size) if lst[p] in single]
        picks = {cand[0], cand[-1]} | set(rng.choice(cand, size=min(3, len(cand)), replace=False).tolist())
        for p in picks:
            j = int(np.searchsorted(rows, lst[p]))
            changed = (zeros == 1) & ~ko.bits[idx[j]]
            assert changed.any(), (name, qi, p, int(lst[p]))
            tried += 1
    assert tried >= 3


# --------------------------------------------------------------------------------------------- (3) the two references agree
@pytest.mark.parametrize("name", ["few_sliced", "plain256_regs", "band_w16_s1", "reads_split_h3", "early_tenth"])
def test_batch_reference_equals_the_per_sequence_reference(name):
    c, ko, queries = build_case(name)
    us, counts = references(name)
    rng = np.random.default_rng(9)
    for qi in sampled_queries(len(queries), rng)[:20]:
        u, cnt = ko.reference(queries[qi])
        assert u == us[qi] and np.array_equal(cnt, counts[qi]), (name, qi)
    # the main query: FULL columns hit, knock-outs do not, and a column counts u minus the k-mers that hold its knocked row
    assert np.array_equal(counts[0] == us[0], ko.knocked < 0)
    per_row = np.array([np.count_nonzero((ko.krows == row).any(axis=1)) for row in ko.R])
    kn = ko.knocked >= 0
    assert np.array_equal(counts[0][kn], us[0] - per_row[ko.knocked[kn]])


# --------------------------------------------------------------------------------------------- (4) routes
@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["route"] is not None])
def test_case_takes_the_route_it_is_built_for(planner, name):
    L, B = planner
    c, ko, queries = build_case(name)
    want, inp = c["route"], kc.planner_input(c, queries)
    kw = c["run_kw"]
    k1 = k1_plan(L, inp["n_seqs"], inp["max_pos"], inp["max_len"], kw.get("k1_global", False))
    head, launches = row_and_plan(L, inp["n_seqs"], inp["wv"], inp["max_pos"], c["h"], kw.get("early_exit", False))
    W, S = c["limits"] or (0, 0)
    band = band_plan(B, inp["n_seqs"], inp["wv"], inp["max_pos"], c["h"], c["m"], kw.get("band_sweep", False), W, S)
    assert k1["route"] == want["k1_route"], (name, k1)
    assert head["too_large"] == 0
    if want["band"]:
        assert band["taken"] == 1 and (band["windows"], band["n_launches"]) == want["band"], (name, band)
        by = kc.BY_K1 if band["windows"] == 1 and k1["route"] == kc.K1_LDS else (kc.SORT1024 if L.launch_host_sort_rows_block(inp["max_pos"], c["h"]) == 1024 else kc.SORT256)
        assert by == want["sorted_by"], name
        # the windows the index was built for are the planner's
        for Wn, shift in c["windows"]:
            assert Wn == W and shift == B.band_host_sort_shift(c["m"], kc.SORT_BUCKETS)
            lo, hi = C.c_uint64(), C.c_uint64()
            for w in (0, 1, Wn // 2, Wn - 1):
                B.band_host_window(C.c_uint64(c["m"]), C.c_uint32(w), C.c_uint32(Wn), C.c_uint32(shift), C.byref(lo), C.byref(hi))
                assert (lo.value, hi.value) == kc.band_window(c["m"], w, Wn, shift)
        return
    assert band["taken"] == 0
    last = launches[-1]
    got = dict(slices=head["slices"], block=launches[0]["block"], tiles=launches[0]["tiles"], n_launches=head["n_launches"],
               last=(last["slices"], last["block"], last["unroll"]))
    for key, v in got.items():
        assert v == want[key], (name, key, v, want[key])
    if want["chunk_q"]:
        assert launches[0]["q1"] - launches[0]["q0"] == want["chunk_q"] and 0 < last["q1"] - last["q0"] < want["chunk_q"], name
    if head["want_sorted"]:
        by = kc.BY_K1 if k1["route"] == kc.K1_LDS else (kc.SORT1024 if L.launch_host_sort_rows_block(inp["max_pos"], c["h"]) == 1024 else kc.SORT256)
    else:
        by = kc.NONE
    assert by == want["sorted_by"], (name, by)
    assert (1 if head["preset"] else 0) == want["preset_by"], name          # (K1's one-launch routes set the words themselves)
    assert head["preset"] == 0 or k1["route"] in (kc.K1_WAVE, kc.K1_LDS)
    # the slices the index was built for are the planner's, the whole batch's or its last launch's
    for S_ in c.get("slices", ()):
        assert S_ in (head["slices"], last["slices"]), name
    # the fused sort's two variants: in registers up to 16 row ids per thread of the workgroup K1 runs in
    if name in ("plain256_regs", "plain256_loop"):
        assert (ko.u * c["h"] <= 16 * 256) == (name == "plain256_regs") and inp["n_seqs"] >= 1024
    if name == "unroll4":
        # the smallest: one query fewer keeps 8 loads in flight
        _, fewer = row_and_plan(L, inp["n_seqs"] - 1, inp["wv"], inp["max_pos"], c["h"], False)
        assert fewer[-1]["unroll"] == 8 and inp["n_seqs"] * inp["wv"] * 64 > (29 << 19) >= (inp["n_seqs"] - 1) * inp["wv"] * 64


def test_sort_rows_block_and_k1_plan_exports(planner):
    """k_sort_rows runs in 1024 threads from 2048 row ids of the longest query on, in 256 below; k1_plan through the test export
    answers what DESIGN.md states for the routes"""
    L, _ = planner
    assert [L.launch_host_sort_rows_block(p, h) for p, h in ((511, 4), (512, 4), (682, 3), (683, 3), (1, 1), (2048, 1), (2047, 1))] == \
        [256, 1024, 256, 1024, 256, 1024, 256]
    assert k1_plan(L, 1, 64, 94, False)["route"] == kc.K1_WAVE and k1_plan(L, 1, 65, 95, False)["route"] == kc.K1_LDS
    assert k1_plan(L, 1, 64, 94, True)["route"] == kc.K1_GLOBAL
    assert k1_plan(L, 1024, 4096, 4126, False)["route"] == kc.K1_LDS and k1_plan(L, 1024, 4097, 4127, False)["route"] == kc.K1_GLOBAL
    assert k1_plan(L, 32, 286, 316, False)["tab_mult"] == 8 and k1_plan(L, 33, 286, 316, False)["tab_mult"] == 4
    assert kc.k1_table_slots(286, 4) == 2048 and kc.sort_shift(20011, 2048) == 4 and kc.sort_shift(20011, 8192) == 2


# --------------------------------------------------------------------------------------------- (5) the two entry points
def test_library_binds_the_row_and_hooks():
    """The device library exports both entry points with the binding's argument types (loading it needs no GPU); the binding's
    structure has the header's fields in the header's order; NULL arguments and an unknown owner kind are refused before anything is
    read."""
    from bigsi_amd import _lib
    fn, fetch = _lib.lib().bigsi_hip_batch_last_row_and, _lib.lib().bigsi_hip_batch_fetch_rows_sorted
    assert fn.argtypes[:2] == [C.c_void_p, C.c_uint32] and fn.restype == C.c_int and fetch.restype == C.c_int
    src = open(os.path.join(ROOT, "include", "bigsi_hip_testing.h")).read()
    body = re.search(r"typedef struct bigsi_hip_row_and_path \{\s*uint32_t ([^;]+);\s*\} bigsi_hip_row_and_path;", src).group(1)
    assert [f.strip() for f in body.split(",")] == [name for name, _ in _lib.RowAndPath._fields_]
    assert C.sizeof(_lib.RowAndPath) == 4 * len(_lib.RowAndPath._fields_)
    for name, value in (("NONE", 0), ("K1", 1), ("SORT256", 2), ("SORT1024", 3)):
        assert "#define BIGSI_SORTED_BY_%s %du" % (name, value) in src and getattr(_lib, "SORTED_BY_" + name) == value == getattr(kc, {"K1": "BY_K1"}.get(name, name))
    assert (_lib.K1_ELEMENTS, _lib.K1_WAVE, _lib.K1_LDS, _lib.K1_GLOBAL) == (0, kc.K1_WAVE, kc.K1_LDS, kc.K1_GLOBAL)
    assert re.search(r"enum K1Route \{ K1_ELEMENTS, K1_WAVE, K1_LDS, K1_GLOBAL \};", open(os.path.join(ROOT, "bigsi_amd", "csrc", "bigsi_launch.hpp")).read())
    out, shift, rows = _lib.RowAndPath(), C.c_uint32(), np.zeros(4, np.uint64)
    assert fn(None, 0, C.byref(out)) == _lib.ERR_INVALID and fn(C.byref(out), 0, None) == _lib.ERR_INVALID
    assert fetch(None, 0, rows.ctypes.data_as(C.c_void_p), 4, C.byref(shift)) == _lib.ERR_INVALID
