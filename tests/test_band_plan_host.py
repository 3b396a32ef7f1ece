"""CPU-only: the band sweep's planner (plan_band_sweep, band_window, band_lower_bound in bigsi_amd/csrc/bigsi_launch.hpp) compiled as
plain host C++ (tests/c_host/band_plan_host.cpp): the shapes the header states, pinned, and the invariants over a seeded sweep of
geometries.  A GPU test compares results, which a slip in the rule leaves right.  The window bounds and the list search also run in a
stand-alone program under AddressSanitizer and UBSan (tests/c_host/band_sanitize_main.cpp)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEAD = ("taken", "windows", "segs_per_launch", "seg_groups", "unroll", "grid", "in_flight", "n_launches", "merge_tail")
LAUNCH = ("seg0", "nseg", "window", "grid", "unroll")
C3, SHARD, KBP = 1563, 977, 970          # result words of 100 000 / 62 500 samples; k-mer positions of a 1 kbp query
M_C3, M_SHARD = 10_000_000, 25_000_000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("band_host") / "libband_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "band_plan_host.cpp")])
    L = C.CDLL(so)
    L.band_host_plan.restype = C.c_uint64
    L.band_host_sort_shift.restype = C.c_uint32
    L.band_host_lower_bound.restype = C.c_uint64
    return L


def plan(L, n_seqs, wv, max_pos, h, m, exact=True, no_sort=False, early_exit=False, forced=False, windows=0, segs=0, cap=1 << 16):
    head, rec = np.zeros(len(HEAD), np.uint64), np.zeros((cap, len(LAUNCH)), np.uint64)
    n = L.band_host_plan(C.c_uint32(n_seqs), C.c_uint64(wv), C.c_uint64(max_pos), C.c_uint32(h), int(exact), int(no_sort), int(early_exit),
                         C.c_uint64(m), int(forced), C.c_uint32(windows), C.c_uint32(segs), head.ctypes.data_as(C.c_void_p),
                         rec.ctypes.data_as(C.c_void_p), C.c_uint64(cap))
    return dict(zip(HEAD, map(int, head))), [dict(zip(LAUNCH, map(int, r))) for r in rec[:min(n, cap)]]


def window(L, m, w, W, shift):
    lo, hi = C.c_uint64(), C.c_uint64()
    L.band_host_window(C.c_uint64(m), C.c_uint32(w), C.c_uint32(W), C.c_uint32(shift), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def test_shipped_constants(lib):
    """What profiles/band_sweep_probe.txt chose: 2 loads in flight, one segment per launch, one window up to 4096 queries and 4 beyond,
    the route from rho = 1.0 and 3072 queries on, at most 16 MiB in flight; and what the library's own step chose: a last segment of
    at most 32 words rides with its neighbour."""
    out = np.zeros(9, np.uint64)
    lib.band_host_constants(out.ctypes.data_as(C.c_void_p))
    assert out.tolist() == [2, 1, 4, 4096, 1000, 16 << 20, 1 << 16, 32, 3072]


def test_pinned_shapes(lib):
    # the C3 stream chunk of 4096 x 1 kbp at h = 4 (rho 1.59): taken, one window, 11 bands of 1024 workgroups (8 MiB in flight) and the
    # 13th segment's 27 words in the 12th's launch
    head, ls = plan(lib, 4096, C3, KBP, 4, M_C3)
    assert head == dict(taken=1, windows=1, segs_per_launch=1, seg_groups=12, unroll=2, grid=1024, in_flight=8 << 20, n_launches=12, merge_tail=1)
    assert ls == [dict(seg0=s, nseg=1, window=0, grid=1024, unroll=2) for s in range(11)] + [dict(seg0=11, nseg=2, window=0, grid=2048, unroll=2)]
    # ... a last segment of 33 words keeps its own launch, and so does any with forced segments
    assert plan(lib, 4096, 1536 + 33, KBP, 4, M_C3)[0]["n_launches"] == 13 and plan(lib, 4096, 1536 + 32, KBP, 4, M_C3)[0]["n_launches"] == 12
    assert plan(lib, 4096, C3, KBP, 4, M_C3, segs=1)[0]["n_launches"] == 13
    # a whole step of 8192 in one batch (rho 3.18): 4 windows per band, at the in-flight cap
    head, ls = plan(lib, 8192, C3, KBP, 4, M_C3)
    assert (head["taken"], head["windows"], head["n_launches"], head["grid"], head["in_flight"], head["merge_tail"]) == (1, 4, 52, 2048, 16 << 20, 0)
    assert [(l["seg0"], l["window"]) for l in ls[:5]] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)]
    # ... and one query more is over the cap
    assert not plan(lib, 8193, C3, KBP, 4, M_C3)[0]["taken"]
    # 1024 queries (rho 0.40, 18 % repeats): below the break-even of 1.0
    assert not plan(lib, 1024, C3, KBP, 4, M_C3)[0]["taken"]
    # rho at and just below 1.0: 4096 x 970 x 4 = 15 892 480 references
    assert plan(lib, 4096, C3, KBP, 4, 15_892_480)[0]["taken"] and not plan(lib, 4096, C3, KBP, 4, 15_892_481)[0]["taken"]
    # fewer than 3072 queries do not fill a launch, whatever rho (256 queries on a 400 000-row cut of the C4 shard: rho 1.86)
    assert plan(lib, 3072, C3, KBP, 4, M_C3)[0]["taken"] and not plan(lib, 3071, C3, KBP, 4, M_C3)[0]["taken"]
    assert not plan(lib, 256, SHARD, KBP, 3, 400_000)[0]["taken"] and not plan(lib, 2048, C3, KBP, 4, 1_000_000)[0]["taken"]
    # 256 queries on the 62.5 k-sample shard at m = 25 M (rho 0.04), and a single query
    assert not plan(lib, 256, SHARD, KBP, 4, M_SHARD)[0]["taken"]
    assert not plan(lib, 1, C3, KBP, 4, M_C3)[0]["taken"]
    # never on the counting path, with early exit or with hash-ordered lists, forced or not
    for kw in (dict(exact=False), dict(early_exit=True), dict(no_sort=True)):
        assert not plan(lib, 4096, C3, KBP, 4, M_C3, **kw)[0]["taken"]
        assert not plan(lib, 4096, C3, KBP, 4, M_C3, forced=True, **kw)[0]["taken"]
    # read-length queries (93 rows: lists that plan_row_and leaves unsorted) and small batches (sliced): not taken unless forced
    assert not plan(lib, 4096, 157, 31, 3, 1009)[0]["taken"] and plan(lib, 4096, 157, 400, 3, 1009)[0]["taken"]
    assert not plan(lib, 301, 130, 70, 3, 1009)[0]["taken"]
    head, ls = plan(lib, 301, 130, 70, 3, 1009, forced=True, windows=3, segs=2)
    assert head == dict(taken=1, windows=3, segs_per_launch=2, seg_groups=1, unroll=2, grid=151, in_flight=602 * 2048, n_launches=3, merge_tail=0)
    assert ls == [dict(seg0=0, nseg=2, window=w, grid=151, unroll=2) for w in range(3)]


def test_invariants_over_a_seeded_sweep(lib):
    """The launches cover every (segment, window) exactly once, a group's windows in ascending order; grids fit a launch and hold a
    wavefront per (query, segment); a plan that is taken unforced stays under the in-flight cap it states."""
    rng = random.Random(7)
    taken = merged = 0
    for _ in range(1500):
        n_seqs, wv = rng.choice([1, 8, 301, 1000, 3071, 3072, 4096, 5000, 8192, 20000]), rng.choice([1, 2, 128, 129, 130, 160, 161, 313, 977, 1563, 4000])
        max_pos, h, m = rng.choice([1, 70, 300, 970, 5000]), rng.choice([1, 3, 4]), rng.choice([1009, 100003, M_C3, M_SHARD])
        forced, windows, segs = rng.random() < 0.5, rng.choice([0, 0, 1, 3, 16, 2000]), rng.choice([0, 1, 2])
        head, ls = plan(lib, n_seqs, wv, max_pos, h, m, forced=forced, windows=windows, segs=segs, cap=1 << 17)
        if not head["taken"]:
            assert head["n_launches"] == 0 and ls == []
            continue
        taken += 1
        W, S = head["windows"], head["segs_per_launch"]
        assert W == (windows or (1 if n_seqs <= 4096 else 4)) and S == (segs or 1) and head["unroll"] == 2
        n_segs, tail = -(-wv // 128), head["merge_tail"]
        assert tail == (segs == 0 and W == 1 and n_segs >= 2 and wv - (n_segs - 1) * 128 <= 32 and n_seqs * 4096 <= 16 << 20)
        merged += tail
        assert head["seg_groups"] == -(-n_segs // S) - tail and head["n_launches"] == head["seg_groups"] * W == len(ls)
        assert [(l["seg0"], l["window"]) for l in ls] == [(g * S, w) for g in range(head["seg_groups"]) for w in range(W)]
        covered = []
        for j, l in enumerate(ls):
            last = tail and j == len(ls) - 1
            assert l["nseg"] == (2 if last else S) and l["unroll"] == 2 and l["grid"] == head["grid"] * (2 if last else 1) <= 2**31 - 1
            assert l["grid"] * 4 >= n_seqs * l["nseg"]
            covered += [(s_, l["window"]) for s_ in range(l["seg0"], l["seg0"] + l["nseg"]) if s_ < n_segs]
        assert sorted(covered) == [(s_, w) for s_ in range(n_segs) for w in range(W)]          # every (segment, window) exactly once
        assert head["grid"] == -(-n_seqs * S // 4) and head["in_flight"] == n_seqs * S * 2 * 1024
        if not forced:
            assert head["in_flight"] <= 16 << 20 and n_seqs * max_pos * h >= m and n_seqs >= 3072
    assert taken > 300 and merged > 20


def test_windows_partition_the_rows(lib):
    """For m not a multiple of W, W > m and every sort shift: window 0 starts at row 0, every window starts where the one before
    ended, the last ends at m, and every inner bound is a whole number of sort buckets."""
    for m in (1, 2, 7, 1009, 8193, 100003, M_C3):
        for buckets in (2, 512, 8192):
            shift = lib.band_host_sort_shift(C.c_uint64(m), C.c_uint64(buckets))
            assert (m - 1) >> shift < buckets and (shift == 0 or (m - 1) >> (shift - 1) >= buckets)
            for W in (1, 2, 3, 16, 64, 2000):
                at = 0
                for w in range(W):
                    lo, hi = window(lib, m, w, W, shift)
                    assert lo == at and lo <= hi <= m and (hi == m or hi % (1 << shift) == 0), (m, W, w)
                    at = hi
                assert at == m
    assert [window(lib, 10, w, 4, 0) for w in range(4)] == [(0, 2), (2, 5), (5, 7), (7, 10)]
    assert [window(lib, 1009, w, 3, 1) for w in range(3)] == [(0, 336), (336, 672), (672, 1009)]      # 505 buckets of 2 rows


def test_list_search(lib):
    """band_lower_bound on a bucket-sorted list (ascending in id >> shift, any order inside a bucket) and bucket-aligned keys."""
    rng = np.random.default_rng(5)
    for shift in (0, 3):
        ids = np.sort(rng.integers(0, 1009, 300).astype(np.uint64))
        if shift:
            for b in np.unique(ids >> np.uint64(shift)):
                sel = np.flatnonzero((ids >> np.uint64(shift)) == b)
                ids[sel] = rng.permutation(ids[sel])
        for key in list(range(0, 1009, 1 << shift)) + [1009]:
            got = lib.band_host_lower_bound(ids.ctypes.data_as(C.c_void_p), C.c_uint64(ids.size), C.c_uint64(key))
            assert got == int((ids < key).sum()), (shift, key)
    assert lib.band_host_lower_bound(None, C.c_uint64(0), C.c_uint64(5)) == 0


def test_library_binds_the_band_hooks():
    """The device library exports bigsi_hip_band_set_limits with the binding's argument types (loading it needs no GPU), and the force
    flag takes the next free bit."""
    from bigsi_amd import _lib
    fn = _lib.lib().bigsi_hip_band_set_limits
    assert fn.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32] and fn.restype == C.c_int
    assert _lib.RUN_BAND_SWEEP == 512
    src = open(os.path.join(ROOT, "include", "bigsi_hip_testing.h")).read()
    assert "#define BIGSI_RUN_BAND_SWEEP 512u" in src


def test_sanitized_program_over_windows_search_and_planner(tmp_path):
    """tests/c_host/band_sanitize_main.cpp -- a program with its own main that replays a band's windows over seeded bucket-sorted
    lists as the kernel does -- built with AddressSanitizer and UBSan and run as a program: it must end clean."""
    exe = str(tmp_path / "band_sanitize")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "c_host", "band_sanitize_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "band windows, search and planner: ok" and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
