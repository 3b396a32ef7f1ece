"""CPU-only: the cut rule of the streamed search (stream_limits, stream_chunk_end, stream_round_to_launches in
bigsi_amd/csrc/bigsi_launch.hpp) compiled as plain host C++ (tests/c_host/stream_plan_host.cpp) against the Python restatement of the
loop it was moved out of (tests/stream_ref.py): the edges of the rule, the shapes of the real constants, a seeded sweep.  The
restatement's band decision is compared with the compiled plan_band_sweep (tests/c_host/band_plan_host.cpp).  A GPU test compares
results, which do not depend on where the cuts fall.  The same functions also run in a stand-alone program under AddressSanitizer and
UBSan (tests/c_host/stream_sanitize_main.cpp)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import stream_ref
from conftest import ROOT

K = 31
C3 = 1563                   # result words of 100 000 samples


def _build(tmp_path_factory, name, src):
    so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", so, os.path.join(ROOT, "tests", "c_host", src)])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = _build(tmp_path_factory, "stream_host", "stream_plan_host.cpp")
    L.stream_host_round.restype = C.c_uint64
    L.stream_host_launch_queries.restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def band_lib(tmp_path_factory):
    L = _build(tmp_path_factory, "band_host2", "band_plan_host.cpp")
    L.band_host_plan.restype = C.c_uint64
    return L


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)


def limits(L, threshold, scored=False, force_counts=False, over=(0, 0, 0)):
    out = np.zeros(6, np.uint64)
    L.stream_host_limits(C.c_double(threshold), int(scored), int(force_counts), C.c_uint64(over[0]), C.c_uint64(over[1]), C.c_uint64(over[2]),
                         out.ctypes.data_as(C.c_void_p))
    return dict(zip(("small_pos", "large_pos", "seqs", "small_chunks", "band_chunks", "chunk_pos"), map(int, out)))


def chunk_end(L, off, nxt, k, limit_pos, limit_seqs):
    """(end, pos, max_pos), or None for the decreasing-offsets error"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    out = np.zeros(4, np.uint64)
    L.stream_host_chunk_end(off.ctypes.data_as(C.c_void_p), C.c_uint64(off.size - 1), C.c_uint64(nxt), C.c_uint32(k), C.c_uint64(limit_pos),
                            C.c_uint64(limit_seqs), out.ctypes.data_as(C.c_void_p))
    return None if out[3] else (int(out[0]), int(out[1]), int(out[2]))


def rounded(L, n, launch_q, more_follow, exact, band):
    return L.stream_host_round(C.c_uint64(n), C.c_uint32(launch_q), int(more_follow), int(exact), int(band))


def header_cuts(L, lengths, threshold, wv, scored=False, force_counts=False, over=(0, 0, 0), band=lambda n, max_pos: False):
    """the loop of search_stream_impl over the compiled functions: [(first, band, n)]"""
    off = offsets_of(lengths)
    lim = limits(L, threshold, scored, force_counts, over)
    launch_q = L.stream_host_launch_queries(C.c_uint64(wv))
    out, nxt, n_seqs = [], 0, len(lengths)
    while nxt < n_seqs:
        taken = False
        if lim["band_chunks"]:
            end, pos, max_pos = chunk_end(L, off, nxt, K, lim["large_pos"], lim["seqs"])
            taken = band(end - nxt, max_pos)
        if not taken:
            end, pos, max_pos = chunk_end(L, off, nxt, K, lim["chunk_pos"], lim["seqs"])
        end = nxt + rounded(L, end - nxt, launch_q, end < n_seqs, threshold == 1.0, taken)
        out.append((nxt, taken, end - nxt))
        nxt = end
    return out


def ref_cuts(lengths, threshold, n_cols, **kw):
    return [(f, b, n) for f, b, n, _ in stream_ref.cuts(lengths, K, threshold, n_cols, 4, 10_000_000, **kw)]


def test_shipped_constants(lib):
    out = np.zeros(4, np.uint64)
    lib.stream_host_constants(out.ctypes.data_as(C.c_void_p))
    assert out.tolist() == [1 << 20, 1 << 22, 4096, 4]
    assert [stream_ref.CHUNK_POSITIONS, stream_ref.LARGE_CHUNK_POSITIONS, stream_ref.CHUNK_SEQS, stream_ref.SLOTS] == out.tolist()


def test_limits_by_stream_kind_and_overrides(lib):
    for thr in (1.0, 0.999999, 0.45, 0.0):
        for scored in (False, True):
            for force in (False, True):
                for over in ((0, 0, 0), (2000, 8000, 64), (0, 8000, 0), (2000, 0, 0), (0, 0, 1), (0, 0, 4096), (5, 3, 4097), (0, 0, 1 << 40)):
                    got = limits(lib, thr, scored, force, over)
                    assert got == {k_: int(v) for k_, v in stream_ref.limits(thr, scored, force, *over).items()}, (thr, scored, force, over)
    # exact and scored streams cut small, thresholded ones large; only an exact unscored stream without forced counts tries the band sweep
    assert limits(lib, 1.0)["chunk_pos"] == 1 << 20 and limits(lib, 0.4)["chunk_pos"] == 1 << 22 and limits(lib, 0.4, scored=True)["chunk_pos"] == 1 << 20
    assert [limits(lib, *a)["band_chunks"] for a in ((1.0,), (1.0, True), (1.0, False, True), (0.4,))] == [1, 0, 0, 0]
    # an override never raises the sequence cap (the workspaces are sized for 4096)
    assert limits(lib, 1.0, over=(0, 0, 4097))["seqs"] == 4096 and limits(lib, 1.0, over=(0, 0, 16))["seqs"] == 16


def test_a_sequence_of_exactly_the_limit_stays_and_one_more_starts_the_next_chunk(lib):
    limit = 500
    for last, want_end in ((limit - 140 + K - 1, 3), (limit - 140 + K, 2)):          # 70 + 70 + (360 | 361) positions
        off = offsets_of([100, 100, last, 100])
        end, pos, max_pos = chunk_end(lib, off, 0, K, limit, 4096)
        assert end == want_end and pos == (limit if want_end == 3 else 140) and max_pos == (360 if want_end == 3 else 70)
        assert (end, pos, max_pos) == stream_ref.chunk_end(off.tolist(), 4, 0, K, limit, 4096)
    # a single sequence of exactly the limit after nothing, and of limit + 1: both are the whole chunk when alone at its start
    for n in (limit, limit + 1):
        off = offsets_of([n + K - 1, 100])
        assert chunk_end(lib, off, 0, K, limit, 4096) == (1, n, n)
        assert chunk_end(lib, off, 1, K, limit, 4096) == (2, 70, 70)


def test_a_first_sequence_over_the_limit_is_a_chunk_of_one(lib):
    off = offsets_of([5030, 5030, 100, 5030])
    assert chunk_end(lib, off, 0, K, 2000, 4096) == (1, 5000, 5000)
    assert chunk_end(lib, off, 1, K, 2000, 4096) == (2, 5000, 5000)
    assert chunk_end(lib, off, 2, K, 2000, 4096) == (3, 70, 70)          # the long one behind it starts its own
    assert chunk_end(lib, off, 3, K, 2000, 4096) == (4, 5000, 5000)


def test_sequences_without_a_kmer_count_one_position_each(lib):
    """shorter than k, empty, exactly k - 1, "ACGT": each adds max(n, 1) = 1 to pos and nothing to what is compared with the limit"""
    off = offsets_of([K - 2, 0, K - 1, 4])
    assert chunk_end(lib, off, 0, K, 2000, 4096) == (4, 4, 0)
    # ... the one it adds counts for those behind it: a chunk filled to the limit takes one such sequence (70 + 0 <= 70) and no second
    off = offsets_of([100] + [0] * 50 + [100])
    assert chunk_end(lib, off, 0, K, 70, 4096) == (2, 71, 70)
    assert chunk_end(lib, off, 0, K, 100, 4096) == (32, 101, 70)          # 70 + 30 x 1, 100 + 0 <= 100 takes the 31st, 101 > 100 ends it
    assert chunk_end(lib, off, 0, K, 100, 16) == (16, 85, 70)
    assert chunk_end(lib, off, 1, K, 10, 4096) == (12, 11, 0)             # eleven of them reach 11 > 10
    # exactly k is one position
    assert chunk_end(lib, offsets_of([K]), 0, K, 1, 1) == (1, 1, 1)


def test_sequence_cap_against_position_limit(lib):
    reads = offsets_of([40] * 100)                                        # 10 positions each
    assert chunk_end(lib, reads, 0, K, 2000, 16) == (16, 160, 10)         # the cap first
    assert chunk_end(lib, reads, 0, K, 155, 16) == (15, 150, 10)          # the positions first
    assert chunk_end(lib, reads, 0, K, 160, 16) == (16, 160, 10)          # both at once
    assert chunk_end(lib, reads, 96, K, 2000, 16) == (100, 40, 10)        # the input ends
    assert chunk_end(lib, offsets_of([100]), 0, K, 2000, 64) == (1, 70, 70)          # n_seqs = 1
    assert chunk_end(lib, offsets_of([]), 0, K, 2000, 64) == (0, 0, 0)


def test_rounding_to_whole_launches(lib):
    for launch_q in (8, 128, 768):
        for n in (1, launch_q - 1, launch_q, 2 * launch_q - 1, 2 * launch_q, 2 * launch_q + 1, 3 * launch_q - 1, 5 * launch_q + 57, 4096):
            want = n // launch_q * launch_q if n >= 2 * launch_q else n
            assert rounded(lib, n, launch_q, True, True, False) == want == stream_ref.round_to_launches(n, launch_q, True, True, False)
            assert want % launch_q == 0 or want == n
            # the last chunk, a thresholded chunk and a band chunk are never rounded
            for more, exact, band in ((False, True, False), (True, False, False), (True, True, True), (False, False, True)):
                assert rounded(lib, n, launch_q, more, exact, band) == n == stream_ref.round_to_launches(n, launch_q, more, exact, band)


def test_launch_queries_equal_the_restatement(lib):
    for wv in list(range(0, 700)) + [977, C3, 4000, 65536, 1 << 22]:
        assert lib.stream_host_launch_queries(C.c_uint64(wv)) == stream_ref.exact_launch_queries(wv), wv
    assert lib.stream_host_launch_queries(C.c_uint64(C3)) == 128 and lib.stream_host_launch_queries(C.c_uint64(313)) == 768


def test_decreasing_offsets(lib):
    first = np.array([100, 99, 300, 400], np.uint64)
    assert chunk_end(lib, first, 0, K, 1 << 20, 4096) is None
    with pytest.raises(stream_ref.DecreasingOffsets):
        stream_ref.chunk_end(first.tolist(), 3, 0, K, 1 << 20, 4096)
    later = np.array([0, 100, 200, 300, 299, 400], np.uint64)
    assert chunk_end(lib, later, 0, K, 1 << 20, 4096) is None
    assert chunk_end(lib, later, 0, K, 140, 4096) == (2, 140, 70)          # a chunk that ends before the bad pair does not see it
    assert chunk_end(lib, later, 2, K, 140, 4096) is None
    assert chunk_end(lib, later, 4, K, 140, 4096) == (5, 71, 71)           # ... and one that starts behind it neither
    with pytest.raises(stream_ref.DecreasingOffsets):
        stream_ref.chunk_end(later.tolist(), 5, 2, K, 140, 4096)


def test_the_real_constants(lib):
    """The shapes the loop's notes speak of, on 100 000 samples (launches of 128 queries)."""
    # 8192 x 1 kbp at 1.0, band sweep not taken: 2^20 positions are 1081 queries of 970 -> 1024 = 8 launches; the last chunk keeps its 24
    got = header_cuts(lib, [1000] * 8192, 1.0, C3)
    assert got == [(1024 * i, False, 1024) for i in range(8)] == ref_cuts([1000] * 8192, 1.0, 100_000, flags_no_sort=True)
    got = header_cuts(lib, [1000] * 9300, 1.0, C3)
    assert got[-2:] == [(8192, False, 1024), (9216, False, 84)] and len(got) == 10
    assert header_cuts(lib, [1000] * 8216, 1.0, C3)[-1] == (7168, False, 1048)          # what fits the limit and ends the input is not rounded
    # ... taken (the large limit holds 4323 of them: the cap of 4096 comes first): two band chunks, not rounded
    band = lambda n, max_pos: stream_ref.band_plan(n, C3, max_pos, 4, 10_000_000)[0]
    assert header_cuts(lib, [1000] * 8192, 1.0, C3, band=band) == [(0, True, 4096), (4096, True, 4096)] == ref_cuts([1000] * 8192, 1.0, 100_000)
    # ... and a remainder the band sweep declines (fewer than 3072 queries) is cut again at the small limit
    assert header_cuts(lib, [1000] * 6000, 1.0, C3, band=band) == [(0, True, 4096), (4096, False, 1024), (5120, False, 880)] == ref_cuts([1000] * 6000, 1.0, 100_000)
    # with forced counts no chunk is tried for it
    assert header_cuts(lib, [1000] * 8192, 1.0, C3, force_counts=True, band=band) == [(1024 * i, False, 1024) for i in range(8)] == ref_cuts([1000] * 8192, 1.0, 100_000, flags_force_counts=True)
    # 1 kbp at 0.4: the sequence cap before the 2^22 positions, never rounded
    assert header_cuts(lib, [1000] * 9000, 0.4, C3, band=band) == [(0, False, 4096), (4096, False, 4096), (8192, False, 808)] == ref_cuts([1000] * 9000, 0.4, 100_000)
    # 61 bp reads: chunks of 4096 (126 976 positions); 4096 is a multiple of the launch size, so rounding changes nothing
    assert header_cuts(lib, [61] * 10_000, 1.0, C3, band=band) == [(0, False, 4096), (4096, False, 4096), (8192, False, 1808)] == ref_cuts([61] * 10_000, 1.0, 100_000)
    # the scored stream: small chunks at any threshold, rounded only when exact
    assert header_cuts(lib, [1000] * 2500, 0.4, C3, scored=True, band=band) == [(0, False, 1081), (1081, False, 1081), (2162, False, 338)] == ref_cuts([1000] * 2500, 0.4, 100_000, scored=True)
    assert header_cuts(lib, [1000] * 2500, 1.0, C3, scored=True, band=band) == [(0, False, 1024), (1024, False, 1024), (2048, False, 452)] == ref_cuts([1000] * 2500, 1.0, 100_000, scored=True)
    # 20 000 samples (launches of 768 queries): 2^20 positions are 2092 queries of 531 bp -> 1536; thresholded: the cap, 4096
    assert header_cuts(lib, [531] * 5000, 1.0, 313) == [(0, False, 1536), (1536, False, 1536), (3072, False, 1928)]
    assert header_cuts(lib, [531] * 5200, 1.0, 313) == [(0, False, 1536), (1536, False, 1536), (3072, False, 1536), (4608, False, 592)]
    assert header_cuts(lib, [531] * 9000, 0.45, 313) == [(0, False, 4096), (4096, False, 4096), (8192, False, 808)]


def test_seeded_sweep_against_the_restatement(lib, band_lib):
    rng = random.Random(11)
    head, rec = np.zeros(9, np.uint64), np.zeros((1, 5), np.uint64)
    chunks = banded = 0
    for it in range(300):
        kind = rng.choice(["reads", "genes", "mixed", "tiny"])
        n = rng.choice([1, 2, 17, 300, 3000])
        lengths = [{"reads": lambda: rng.randint(31, 90), "genes": lambda: rng.randint(300, 1200), "mixed": lambda: rng.choice([0, 4, 30, 31, 100, 5030]),
                    "tiny": lambda: rng.randint(0, 40)}[kind]() for _ in range(n)]
        over = rng.choice([(0, 0, 0), (2000, 8000, 64), (70, 71, 16), (1, 1, 1), (100_000, 400_000, 0), (0, 0, 5)])
        thr, scored, force, forced_band = rng.choice([1.0, 1.0, 0.45]), rng.random() < 0.2, rng.random() < 0.2, rng.random() < 0.5
        n_cols, h, m = rng.choice([333, 8261, 20_000, 100_000]), rng.choice([1, 3, 4]), rng.choice([1009, 200_003])
        wv = -(-n_cols // 64)

        def band(nq, max_pos):
            got = band_lib.band_host_plan(C.c_uint32(nq), C.c_uint64(wv), C.c_uint64(max_pos), C.c_uint32(h), 1, 0, 0, C.c_uint64(m), int(forced_band),
                                          C.c_uint32(0), C.c_uint32(0), head.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), C.c_uint64(1))
            assert (bool(head[0]), int(got)) == stream_ref.band_plan(nq, wv, max_pos, h, m, forced_band)
            return bool(head[0])

        got = header_cuts(lib, lengths, thr, wv, scored, force, over, band)
        want = [(f, b, c) for f, b, c, _ in stream_ref.cuts(lengths, K, thr, n_cols, h, m, scored, force, forced_band, chunk_positions=over[0],
                                                            large_chunk_positions=over[1], chunk_seqs=over[2])]
        assert got == want, (it, kind, n, over, thr)
        assert got[0][0] == 0 and all(a[0] + a[2] == b[0] for a, b in zip(got, got[1:])) and got[-1][0] + got[-1][2] == n
        chunks += len(got)
        banded += sum(b for _, b, _ in got)
    assert chunks > 3000 and banded > 50


def test_band_restatement_on_the_pinned_shapes(band_lib):
    """stream_ref.band_plan against the compiled planner where tests/test_band_plan_host.py pins it"""
    head, rec = np.zeros(9, np.uint64), np.zeros((1, 5), np.uint64)
    for n, wv, max_pos, h, m, forced, w, s in ((4096, C3, 970, 4, 10_000_000, 0, 0, 0), (8192, C3, 970, 4, 10_000_000, 0, 0, 0), (8193, C3, 970, 4, 10_000_000, 0, 0, 0),
                                               (3072, C3, 970, 4, 10_000_000, 0, 0, 0), (3071, C3, 970, 4, 10_000_000, 0, 0, 0), (4096, C3, 970, 4, 15_892_481, 0, 0, 0),
                                               (4096, 157, 31, 3, 1009, 0, 0, 0), (4096, 157, 400, 3, 1009, 0, 0, 0), (301, 130, 70, 3, 1009, 1, 3, 2),
                                               (301, 130, 70, 3, 1009, 1, 2000, 1), (301, 130, 70, 3, 1009, 1, 0, 0), (3072, 130, 342, 3, 1009, 0, 0, 0),
                                               (3072, 130, 341, 3, 1009, 0, 0, 0), (3072, 6, 342, 3, 1009, 0, 0, 0)):
        got = band_lib.band_host_plan(C.c_uint32(n), C.c_uint64(wv), C.c_uint64(max_pos), C.c_uint32(h), 1, 0, 0, C.c_uint64(m), forced, C.c_uint32(w),
                                      C.c_uint32(s), head.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), C.c_uint64(1))
        assert (bool(head[0]), int(got)) == stream_ref.band_plan(n, wv, max_pos, h, m, bool(forced), w, s), (n, wv, max_pos, m, forced, w, s)
    assert stream_ref.band_plan(3072, 130, 342, 3, 1009) == (True, 1) and not stream_ref.band_plan(3072, 130, 341, 3, 1009)[0]


def test_library_binds_the_stream_hooks():
    """The device library exports the two test entry points with the binding's argument types (loading it needs no GPU), and a NULL
    index is refused."""
    from bigsi_amd import _lib
    L = _lib.lib()
    assert L.bigsi_hip_stream_set_limits.argtypes == [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64] and L.bigsi_hip_stream_set_limits.restype == C.c_int
    assert L.bigsi_hip_stream_last_chunks.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    assert L.bigsi_hip_stream_set_limits(None, 0, 0, 0) == _lib.ERR_INVALID
    n = C.c_uint64(7)
    assert L.bigsi_hip_stream_last_chunks(None, None, None, 0, C.byref(n)) == _lib.ERR_INVALID
    src = open(os.path.join(ROOT, "include", "bigsi_hip_testing.h")).read()
    assert "bigsi_hip_stream_set_limits" in src and "bigsi_hip_stream_last_chunks" in src


def test_sanitized_program_over_cuts_rounding_and_limits(tmp_path):
    """tests/c_host/stream_sanitize_main.cpp -- a program with its own main that replays the stream's loop over seeded offset arrays
    -- built with AddressSanitizer and UBSan and run as a program: it must end clean."""
    exe = str(tmp_path / "stream_sanitize")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "c_host", "stream_sanitize_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "stream cuts, rounding and limits: ok" and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
