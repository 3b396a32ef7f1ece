"""The k-mer counter's host-only planners without a GPU (csrc/bigsi_launch.hpp, compiled by g++ through tests/c_host/kmercount_plan_host.cpp):
plan_kmer_count_add -- a call's positions, its refusal at the lifetime bound and at decreasing offsets, and the staging chunks: cut at
read boundaries, a longer read cut with a k - 1 byte overlap, the ranges covering exactly the bytes the offsets name -- against the
Python restatement (tests/kmercount_ref.py) over the cut pieces; plan_kmer_table -- powers of two, load at most 1/2 --; and the same
file as a stand-alone sanitized program that is handed a nine-byte heap buffer with the refused offsets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmercount_ref as R
from conftest import ROOT
from raw_index import ptr

SRC = os.path.join(ROOT, "tests", "c_host", "kmercount_plan_host.cpp")
LIFETIME = (1 << 32) - 1
LIMITS = (64, 100, 4096)
NONE, NOT_MONOTONE, OVER_LIFETIME = 0, 1, 2


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("kmercount_plan") / "libkmercount_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", so, SRC])
    lib = C.CDLL(so)
    u64, P = C.c_uint64, C.c_void_p
    lib.kc_plan_add.argtypes, lib.kc_plan_add.restype = [C.c_uint32, P, u64, u64, u64, P, P, u64], u64
    lib.kc_plan_table.argtypes = [u64, u64, u64, u64, P]
    lib.kc_initial_slots.argtypes, lib.kc_initial_slots.restype = [u64, u64], u64
    lib.kc_host_add.argtypes, lib.kc_host_add.restype = [C.c_uint32, C.c_char_p, P, u64, u64, u64, P], C.c_int
    return lib


def plan_add(lib, k, offsets, taken=0, limit=1 << 26, capacity=4096):
    off = np.asarray(offsets, np.uint64)
    head, chunks = np.zeros(3, np.uint64), np.zeros(6 * capacity, np.uint64)
    n = lib.kc_plan_add(k, ptr(off), len(off) - 1, taken, limit, ptr(head), ptr(chunks), capacity)
    names = ("begin", "end", "seq0", "seq1", "positions", "staged")
    return int(head[0]), int(head[1]), int(head[2]), [dict(zip(names, (int(x) for x in chunks[6 * i:6 * i + 6]))) for i in range(min(n, capacity))], n


def offsets_of(seqs, base=0):
    return [base] + [base + int(x) for x in np.cumsum([len(s) for s in seqs])]


def test_constants(plan_lib):
    c = np.zeros(8, np.uint64)
    plan_lib.kc_constants(ptr(c))
    lifetime, chunk, min_chunk, slots, min_slots, tile, lane, block = (int(x) for x in c)
    assert lifetime == LIFETIME and min_chunk == 64 >= 2 * R.MAX_K and chunk >= min_chunk
    assert slots & (slots - 1) == 0 and min_slots == 64 and tile == block * lane == 4096 and lane == 16


def test_positions_and_refusals(plan_lib):
    k = 5
    # 2^32 + 4 bytes are 2^32 windows of k = 5: one more than a counter takes; 2^32 + 3 bytes are exactly what it takes
    refusal, _, positions, chunks, n = plan_add(plan_lib, k, [0, (1 << 32) + 4])
    assert (refusal, positions, chunks, n) == (OVER_LIFETIME, 1 << 32, [], 0)
    refusal, _, positions, chunks, n = plan_add(plan_lib, k, [0, (1 << 32) + 3])
    assert (refusal, positions) == (NONE, LIFETIME) and n == len(chunks) > 0 and sum(c["positions"] for c in chunks) == LIFETIME
    assert chunks[0]["begin"] == 0 and chunks[-1]["end"] == (1 << 32) + 3
    # with 5 positions taken: the claim that is one over, and the exact fit
    fit = LIFETIME - 5 + k - 1
    assert plan_add(plan_lib, k, [0, fit + 1], taken=5)[0] == OVER_LIFETIME and plan_add(plan_lib, k, [0, fit], taken=5)[:3] == (NONE, 0, LIFETIME - 5)
    assert plan_add(plan_lib, k, [0, 9], taken=LIFETIME - 5)[0] == NONE and plan_add(plan_lib, k, [0, 9], taken=LIFETIME - 4)[0] == OVER_LIFETIME
    assert plan_add(plan_lib, k, [0, 4], taken=LIFETIME)[0] == NONE          # no window: nothing is claimed
    assert plan_add(plan_lib, k, [7, 20, 40, 30])[:2] == (NOT_MONOTONE, 2) and plan_add(plan_lib, k, [9, 0])[:2] == (NOT_MONOTONE, 0)
    assert plan_add(plan_lib, k, [9, 0])[3] == []
    # many reads whose windows sum to one over
    assert plan_add(plan_lib, k, offsets_of([b"A" * 9] * 4), taken=LIFETIME - 19)[0] == OVER_LIFETIME
    assert plan_add(plan_lib, k, offsets_of([b"A" * 9] * 4), taken=LIFETIME - 20)[0] == NONE


def pieces_of(blob, off, chunk):
    """The pieces of a chunk as the stage copies them: the intersections of its range with its reads."""
    out = []
    for i in range(chunk["seq0"], chunk["seq1"]):
        a, b = max(off[i], chunk["begin"]), min(off[i + 1], chunk["end"])
        out.append(blob[a:b] if b > a else b"")
    return out


def check_chunks(k, seqs, limit, chunks, base=0):
    off = offsets_of(seqs, base)
    blob = b"\xee" * base + b"".join(seqs)
    assert chunks[0]["begin"] == off[0] and chunks[-1]["end"] == off[-1]          # exactly the bytes the offsets name
    for c in chunks:
        assert off[0] <= c["begin"] < c["end"] <= off[-1] and c["end"] - c["begin"] <= limit
        assert off[c["seq0"]] <= c["begin"] < max(off[c["seq0"] + 1], c["begin"] + 1) and off[c["seq1"] - 1] <= c["end"] <= off[c["seq1"]]
    for a, b in zip(chunks, chunks[1:]):
        if b["begin"] == a["end"]:
            assert a["end"] in off                                                  # cut at a read boundary
        else:
            assert b["begin"] == a["end"] - (k - 1) and a["end"] not in off         # cut inside a read: the next chunk overlaps by k - 1
            assert a["end"] - a["begin"] == limit
    # the windows of the chunks, counted by the restatement over the cut pieces, are those of the whole
    want = R.count(seqs, k)
    got = R.merge(*[R.count(pieces_of(blob, off, c), k) for c in chunks])
    assert got == want
    for c in chunks:
        pieces = pieces_of(blob, off, c)
        assert c["positions"] == sum(max(len(p) - k + 1, 0) for p in pieces) and c["staged"] == sum(len(p) + 1 for p in pieces if p)


@pytest.mark.parametrize("k", R.LENGTH_KS)
@pytest.mark.parametrize("limit", LIMITS)
def test_chunk_cuts(plan_lib, k, limit):
    seqs = R.length_edge_case(k)
    for base in (0, 13):
        refusal, _, positions, chunks, n = plan_add(plan_lib, k, offsets_of(seqs, base), limit=limit)
        assert refusal == NONE and n == len(chunks) and positions == sum(R.count(seqs, k)[1:])
        check_chunks(k, seqs, limit, chunks, base)
        if limit < R.LONG:
            assert any(b["begin"] != a["end"] for a, b in zip(chunks, chunks[1:]))          # the case holds reads longer than the limit
    # a read of 2 * limit + 3 bytes: cut with an overlap of k - 1, twice or more
    long_read = [R.rand_seq(R.random.Random(limit + k), 2 * limit + 3)]
    chunks = plan_add(plan_lib, k, offsets_of(long_read), limit=limit)[3]
    assert len(chunks) >= 3 and [c["begin"] for c in chunks[:3]] == [0, limit - (k - 1), 2 * (limit - (k - 1))] and chunks[0]["end"] == limit
    check_chunks(k, long_read, limit, chunks)
    # between two short reads, and alone among empty ones
    for seqs in ([b"ACGTA"] + long_read + [b"TTTTTTT"], [b"", b""] + long_read + [b"", b""]):
        check_chunks(k, seqs, limit, plan_add(plan_lib, k, offsets_of(seqs), limit=limit)[3])
    assert plan_add(plan_lib, k, offsets_of([b"", b"", b""]))[3] == [] and plan_add(plan_lib, k, [5])[3] == []          # no bytes, no sequences


def test_host_add_reads_what_the_chunks_name(plan_lib):
    out = np.zeros(2, np.uint64)
    for k in R.LENGTH_KS:
        seqs = R.length_edge_case(k)
        blob, off = b"".join(seqs), np.asarray(offsets_of(seqs), np.uint64)
        for limit in LIMITS:
            assert plan_lib.kc_host_add(k, blob, ptr(off), len(seqs), 0, limit, ptr(out)) == 0
            assert int(out[0]) == int(out[1]) == R.count(seqs, k)[1]
    assert plan_lib.kc_host_add(5, b"ACGTACGTA", ptr(np.array([0, (1 << 32) + 4], np.uint64)), 1, 0, 4096, ptr(out)) == -4
    assert plan_lib.kc_host_add(5, b"ACGTACGTA", ptr(np.array([9, 0], np.uint64)), 1, 0, 4096, ptr(out)) == -1


def test_table_rule(plan_lib):
    out = np.zeros(3, np.uint64)

    def table(slots_now, distinct, positions, staged=0):
        plan_lib.kc_plan_table(slots_now, distinct, positions, staged, ptr(out))
        return int(out[0]), int(out[1]), int(out[2])

    for slots in (64, 1 << 10, 1 << 16, 1 << 30):
        for distinct in (0, 1, slots // 4, slots // 2 - 1, slots // 2):
            fits = slots // 2 - distinct
            assert table(slots, distinct, fits) == (slots, 0, 0)                       # distinct + positions == slots / 2: stays
            assert table(slots, distinct, fits + 1) == (2 * slots, 1, 0)               # one more: doubles
    for slots_now, distinct, positions in ((0, 0, 0), (64, 0, 5000), (100, 7, 0), (1 << 12, 3000, 70000), (64, LIFETIME, LIFETIME), (1 << 20, 0, 1)):
        slots, grow, _ = table(slots_now, distinct, positions)
        assert slots & (slots - 1) == 0 and slots >= max(slots_now, 64) and 2 * (distinct + positions) <= slots and grow == (slots != slots_now)
        floor = 64
        while floor < slots_now:
            floor *= 2
        assert slots == floor or 2 * (distinct + positions) > slots // 2          # no larger than needed: half of it would not do
    assert [table(64, 0, 0, staged)[2] for staged in (0, 1, 4096, 4097, 8192, (32 << 20) * 2)] == [0, 1, 1, 2, 2, 16384]
    assert plan_lib.kc_initial_slots(0, 1 << 16) == 1 << 16 and plan_lib.kc_initial_slots(40000, 1 << 16) == 1 << 17 and plan_lib.kc_initial_slots(5, 64) == 64


def test_the_table_case_grows_and_is_cut_as_the_gpu_test_needs(plan_lib):
    """tests/test_gpu_kmercount.py runs table_case() with a 4096-byte chunk and 64 initial slots: several chunks, several growths."""
    reads = R.table_case() + [R.rand_seq(R.random.Random(77), 9001)]
    chunks = plan_add(plan_lib, R.TABLE_K, offsets_of(reads), limit=4096)[3]
    assert len(chunks) >= 5 and any(b["begin"] != a["end"] for a, b in zip(chunks, chunks[1:]))
    out, slots, distinct, growths = np.zeros(3, np.uint64), 64, 0, 0
    for c in chunks:
        plan_lib.kc_plan_table(slots, distinct, c["positions"], c["staged"], ptr(out))
        growths += int(out[1])
        slots, distinct = int(out[0]), distinct + c["positions"]          # (nearly all windows of the case are distinct)
    assert growths >= 3 and slots >= 1 << 14


def test_sanitized_program_over_the_planner(tmp_path):
    """The same file with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own: it
    passes a nine-byte heap buffer with the refused offsets (2^32 + 4 at k = 5, the one-over claim, a descending pair) -- a clean exit
    shows that no byte of a refused call is read -- and stages accepted calls out of buffers of exactly the bytes named."""
    exe = str(tmp_path / "kmercount_plan_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-DKMERCOUNT_PLAN_MAIN", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "kmercount planner: ok", (r.stdout[-1000:], r.stderr[-3000:])
