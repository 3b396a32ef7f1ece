"""Consensus collapse without a GPU: the CPU twin of bigsi_hip_consensus_columns_into against numpy on the very bits written
(counts[g] = bits[:, group_of == g].sum(axis=1), out[:, g] = counts[g] >= need[g], packed, zero to the stride), the per-call tables of
plan_consensus_columns (csrc/bigsi_launch.hpp, compiled by g++) against a bit-by-bit restatement of the row format -- and the kernel's
own arithmetic replayed from those tables: packed 32-bit adds that wrap like the device's, window by window, then the threshold --,
the field width, window and LDS invariants of the planner, the rule percent -> members (bigsi_amd/consensus.py), what BIGSI.consensus
and its command line decide before any device call, and a stand-alone sanitized program over the planner and the twin."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raw_index import ptr, ragged_bits
from test_collapse_columns_host import DROPPED, collapse_maps, junk_rows, mem_bit, twin_info, twin_open, twin_rows, twin_source
from test_compact_columns_host import WIDTHS

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_STATE = -1, -6
NEVER = 0xFFFFFFFF
DELETED = "D3L3T3D"


def group_sizes(group_of, groups):
    return np.bincount(group_of[group_of != DROPPED].astype(np.int64), minlength=groups).astype(np.int64)


def need_vectors(group_of, groups, seed=0):
    """[(label, need uint32[G])]: every group needs 1 (the OR), its size (the AND; a group without members needs 1 and stays zero),
    and a seeded random number in [1, size + 1] (size + 1: more than there are, a zero column)."""
    sizes = group_sizes(group_of, groups)
    rng = np.random.default_rng(3000 + groups + seed)
    return [("one", np.ones(groups, np.uint32)), ("size", np.maximum(sizes, 1).astype(np.uint32)),
            ("random", (1 + rng.integers(0, sizes + 1)).astype(np.uint32))]


def member_counts(bits, group_of, groups):
    """int64[m, G]: counts[:, g] = bits[:, group_of == g].sum(axis=1), for all groups at once (columns sorted by group, one reduceat)."""
    counts = np.zeros((bits.shape[0], groups), np.int64)
    cols = np.flatnonzero(group_of != DROPPED)
    if cols.size:
        order = cols[np.argsort(group_of[cols], kind="stable")]
        ids = group_of[order].astype(np.int64)
        starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
        counts[:, ids[starts]] = np.add.reduceat(bits[:, order].astype(np.int64), starts, axis=1)
    return counts


def consensus_rows(bits, group_of, groups, need, row_bytes):
    """The numpy model on the very bits written: column g = counts[g] >= need[g], packed, zero up to row_bytes."""
    out = (member_counts(bits, group_of, groups) >= need.astype(np.int64)[None, :]).astype(np.uint8)
    want = np.zeros((bits.shape[0], row_bytes), np.uint8)
    packed = np.packbits(out, axis=1)
    want[:, :packed.shape[1]] = packed
    return want


def test_the_model_is_the_stated_one():
    bits = ragged_bits(19, 200)
    for label, group_of, groups in collapse_maps(200):
        counts = member_counts(bits, group_of, groups)
        for g in range(groups):
            assert np.array_equal(counts[:, g], bits[:, group_of == g].sum(axis=1)), (label, g)


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    L.bigsi_cpu_collapse_columns_into.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.bigsi_cpu_collapse_columns_into.restype = C.c_int32
    L.bigsi_cpu_consensus_columns_into.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.bigsi_cpu_consensus_columns_into.restype = C.c_int32
    return L


@pytest.mark.parametrize("n", WIDTHS)
def test_twin_against_numpy(cpu, n):
    m = 257 if n < 1000 else 41
    bits = ragged_bits(m, n)
    for label, group_of, groups in collapse_maps(n):
        src, written = twin_source(cpu, bits)
        for which, need in need_vectors(group_of, groups):
            dst = twin_open(cpu, m, 0, 1)
            assert cpu.bigsi_cpu_consensus_columns_into(dst, src, ptr(group_of), groups, ptr(need)) == 0, cpu.bigsi_cpu_last_error()
            info = twin_info(cpu, dst)
            assert info.num_cols == groups and info.col_capacity >= groups, (n, label, which)
            for rb in ((groups + 7) // 8, int(info.row_stride_bytes)):          # the stride padding is zero, no junk was counted
                assert np.array_equal(twin_rows(cpu, dst, m, rb), consensus_rows(bits, group_of, groups, need, rb)), (n, label, which, rb)
            if which == "one":          # = the OR collapse of the same map, bit for bit
                orr = twin_open(cpu, m, 0, 1)
                assert cpu.bigsi_cpu_collapse_columns_into(orr, src, ptr(group_of), groups) == 0, cpu.bigsi_cpu_last_error()
                rb = int(info.row_stride_bytes)
                assert twin_info(cpu, orr).row_stride_bytes == rb and np.array_equal(twin_rows(cpu, dst, m, rb), twin_rows(cpu, orr, m, rb)), (n, label)
                assert cpu.bigsi_cpu_close(orr) == 0
            assert cpu.bigsi_cpu_close(dst) == 0
        assert np.array_equal(twin_rows(cpu, src, m, written.shape[1]), written) and twin_info(cpu, src).num_cols == n          # only read
        assert cpu.bigsi_cpu_close(src) == 0


def test_twin_refusals(cpu):
    bits = ragged_bits(64, 100)
    g = (np.arange(100) % 7).astype(np.uint32)
    need = np.full(7, 2, np.uint32)
    src, _ = twin_source(cpu, bits)
    full, _ = twin_source(cpu, bits)
    other_m, other_h, empty = twin_open(cpu, 65, 0, 1), twin_open(cpu, 64, 0, 1, h=2), twin_open(cpu, 64, 0, 1)
    bad = g.copy()
    bad[41] = 7
    zero = need.copy()
    zero[5] = 0
    call = cpu.bigsi_cpu_consensus_columns_into
    for args, want, words in (((None, src, ptr(g), 7, ptr(need)), ERR_INVALID, ()),
                              ((empty, None, ptr(g), 7, ptr(need)), ERR_INVALID, ()),
                              ((empty, src, None, 7, ptr(need)), ERR_INVALID, ()),
                              ((empty, src, ptr(g), 7, None), ERR_INVALID, ()),                           # NULL min_members
                              ((empty, src, ptr(g), 0, ptr(need)), ERR_INVALID, ("0",)),
                              ((empty, src, ptr(g), 0xFFFFFFFF, ptr(need)), ERR_INVALID, ("4294967295",)),
                              ((empty, src, ptr(g), 1 << 40, ptr(need)), ERR_INVALID, ()),
                              ((empty, src, ptr(bad), 7, ptr(need)), ERR_INVALID, ("41", "7")),          # the message names the column and the value
                              ((empty, src, ptr(g), 7, ptr(zero)), ERR_INVALID, ("min_members[5]",)),    # ... and here the group
                              ((src, src, ptr(g), 7, ptr(need)), ERR_INVALID, ()),                       # dst == src
                              ((other_m, src, ptr(g), 7, ptr(need)), ERR_INVALID, ("65", "64")),
                              ((other_h, src, ptr(g), 7, ptr(need)), ERR_INVALID, ("2", "3")),
                              ((full, src, ptr(g), 7, ptr(need)), ERR_STATE, ("100",))):                 # a destination that holds columns
        rc = call(*args)
        msg = cpu.bigsi_cpu_last_error().decode()
        assert rc == want and msg and all(w in msg for w in words), (rc, want, msg)
    for h in (empty, other_m, other_h):          # a refused call left the destination empty
        assert twin_info(cpu, h).num_cols == 0 and not twin_rows(cpu, h, 64, int(twin_info(cpu, h).row_stride_bytes)).any()
    assert twin_info(cpu, full).num_cols == 100
    more = need.copy()
    more[5] = NEVER                              # more members than there are is no bad entry: a zero column
    assert call(empty, src, ptr(g), 7, ptr(more)) == 0 and twin_info(cpu, empty).num_cols == 7
    got = np.unpackbits(twin_rows(cpu, empty, 64, 1), axis=1)
    assert not got[:, 5].any() and got[:, :5].any()
    for h in (src, full, other_m, other_h, empty):
        assert cpu.bigsi_cpu_close(h) == 0


# --------------------------------------------------------------------------------------------- the plan's tables
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("consensus_host") / "libconsensus_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "consensus_host.cpp")])
    lib = C.CDLL(so)
    lib.consensus_host_field_bits.argtypes = [C.c_uint64]
    lib.consensus_host_field_bits.restype = C.c_uint32
    lib.consensus_host_first_zero.argtypes = [C.c_void_p, C.c_uint64]
    lib.consensus_host_first_zero.restype = C.c_uint64
    lib.consensus_host_plan.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.consensus_host_window.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


HEAD = ("src_words", "table_words", "dst_words", "field_bits", "largest", "window_words", "windows", "image_words", "block", "grid", "lds_bytes", "moved",
        "need_entries")
CONSTS = ("dropped", "waves", "window_words", "lds_bytes", "loads", "gathers", "block", "never")


def constants(lib):
    c = np.zeros(8, np.uint64)
    lib.consensus_host_constants(ptr(c))
    return dict(zip(CONSTS, (int(x) for x in c)))


def plan(lib, n, group_of, groups, need=None, m=1000, window=0, tables=True):
    """plan_consensus_columns as a dict: the head, and with `tables` dst_col, live, sizes and (when `need` is given) need."""
    tw, dw2 = ((n + 63) // 64 + 1) // 2 * 2, ((groups + 63) // 64 + 1) // 2 * 2
    head = np.zeros(len(HEAD), np.uint64)
    dst_col, live = np.zeros(max(tw * 64, 1), np.uint32), np.zeros(max(tw, 1), np.uint64)
    sizes, tab = np.zeros(groups if tables else 1, np.uint32), np.zeros(dw2 * 64 if tables else 1, np.uint32)
    args = (ptr(dst_col), tw * 64, ptr(live), tw, ptr(sizes), groups, ptr(tab), dw2 * 64) if tables else (None, 0, None, 0, None, 0, None, 0)
    assert lib.consensus_host_plan(n, ptr(group_of), groups, ptr(need), m, window, ptr(head), *args) == 0
    p = dict(zip(HEAD, (int(x) for x in head)))
    assert p["src_words"] == (n + 63) // 64 and p["table_words"] == tw and p["dst_words"] == (groups + 63) // 64
    assert p["need_entries"] == (dw2 * 64 if need is not None else 0)
    p["dst_col"], p["live"], p["sizes"], p["need"] = dst_col[:tw * 64], live[:tw], sizes, tab
    return p


def runs_of_255(n):
    """Consecutive groups of exactly 255 columns (the last one takes what is left): 8-bit fields at their maximum beside each other."""
    return (np.arange(n) // 255).astype(np.uint32), (n + 254) // 255


@pytest.mark.parametrize("n", WIDTHS)
def test_plan_tables_against_restatement(plan_lib, n):
    assert all(mem_bit(l) == l ^ 7 for l in range(64))                    # (what the kernel's read-out takes for collapse_mem_bit)
    for label, group_of, groups in collapse_maps(n) + [("runs255",) + runs_of_255(n)]:
        need = need_vectors(group_of, groups)[2][1]
        p = plan(plan_lib, n, group_of, groups, need)
        want_col, want_live = np.full(p["table_words"] * 64, DROPPED, np.uint32), [0] * p["table_words"]
        for c in range(n):
            g = int(group_of[c])
            if g == DROPPED:
                continue
            want_col[64 * (c // 64) + mem_bit(c % 64)] = g                # the permutation on the source side only
            want_live[c // 64] |= 1 << mem_bit(c % 64)
        assert np.array_equal(p["dst_col"], want_col), (n, label)
        assert [int(x) for x in p["live"]] == want_live, (n, label)
        assert p["moved"] == int((group_of != DROPPED).sum())
        live_bits = np.unpackbits(p["live"].view(np.uint8), bitorder="little")
        assert np.array_equal(live_bits.astype(bool), p["dst_col"] != DROPPED)
        sizes = group_sizes(group_of, groups)
        assert np.array_equal(p["sizes"], sizes) and p["largest"] == int(sizes.max())
        # need: entry 64 w + l = min_members[64 w + mem_bit(l)], the padding up to the image's extent never reached
        want_need = np.full(p["need_entries"], NEVER, np.uint32)
        for e in range(p["need_entries"]):
            g = 64 * (e // 64) + mem_bit(e % 64)
            if g < groups:
                want_need[e] = need[g]
        assert np.array_equal(p["need"], want_need), (n, label)
        # the invariant behind the packed adds: no count passes its group's size, no size the field's maximum
        assert int(sizes.max()) <= (1 << p["field_bits"]) - 1 and p["field_bits"] in (8, 16, 32)
    z = np.ones(9, np.uint32)
    assert plan_lib.consensus_host_first_zero(ptr(z), 9) == 9
    z[[4, 7]] = 0
    assert plan_lib.consensus_host_first_zero(ptr(z), 9) == 4


def test_field_bits_follow_the_largest_group(plan_lib):
    k = constants(plan_lib)
    for largest, bits in ((0, 8), (1, 8), (255, 8), (256, 16), (65_535, 16), (65_536, 32), (1 << 32, 32)):
        assert plan_lib.consensus_host_field_bits(largest) == bits, largest
    for largest, bits in ((1, 8), (255, 8), (256, 16), (65_535, 16), (65_536, 32)):
        n = largest + 40
        group_of = np.concatenate([np.full(largest, 3, np.uint32), 4 + np.arange(40, dtype=np.uint32) % 5])      # the others are small
        p = plan(plan_lib, n, group_of, 9, tables=False)
        assert (p["field_bits"], p["largest"]) == (bits, max(largest, 8)), largest
        assert p["window_words"] == k["window_words"] // bits and p["window_words"] * 64 == {8: 16_384, 16: 8192, 32: 4096}[bits]


def replay_kernel(lib, p, src_row):
    """k_consensus_columns' arithmetic on one row from the tables: the set bits of (source & live) by their memory bit address, their
    dst_col entries, window by window the ones inside [lo, lo + span) added as 1 << field into an image of packed uint32 words
    (numpy's uint32 adds wrap like the device's), lane l of the read-out of word w taking the field of column 64 w + mem_bit(l)
    against need[64 w + l], the used part of the image cleared.  Returns the destination row's bytes up to round_up(dst_words, 2)
    words."""
    tw, dw, fb = p["table_words"], p["dst_words"], p["field_bits"]
    per, mask = 32 // fb, (1 << fb) - 1
    src_bits = np.unpackbits(src_row[:tw * 8], bitorder="little")         # index = bit address in memory
    live_bits = np.unpackbits(p["live"].view(np.uint8), bitorder="little")
    cols = p["dst_col"][np.flatnonzero(src_bits & live_bits)].astype(np.int64)
    out = np.zeros((dw + 1) // 2 * 2 * 64, np.uint8)
    image = np.zeros(p["image_words"] * 2, np.uint32)
    lane_col = np.array([mem_bit(l) for l in range(64)], np.int64)
    first, count = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    for j in range(p["windows"]):
        lib.consensus_host_window(dw, p["window_words"], j, ptr(first), ptr(count))
        win0, win_n = int(first[0]), int(count[0])
        lo, span = win0 * 64, win_n * 64
        rel = (cols - lo) % (1 << 32)                                     # (the kernel's 32-bit wrap)
        rel = rel[rel < span]
        np.add.at(image, rel // per, (np.uint64(1) << ((rel % per) * fb).astype(np.uint64)).astype(np.uint32))
        pair_n = (win_n + 1) // 2 * 2
        assert pair_n * 2 * fb <= image.size
        c = (np.arange(pair_n, dtype=np.int64)[:, None] * 64 + lane_col[None, :]).ravel()
        have = (image[c // per].astype(np.uint64) >> ((c % per) * fb).astype(np.uint64)) & np.uint64(mask)
        out[lo:lo + pair_n * 64] = have >= p["need"][lo:lo + pair_n * 64].astype(np.uint64)
        image[:pair_n * 2 * fb] = 0
    assert not image.any()
    return np.packbits(out, bitorder="little")


@pytest.mark.parametrize("n", (1, 64, 65, 129, 1025, 8193))
def test_kernel_arithmetic_replayed_from_the_tables(plan_lib, n):
    """What k_consensus_columns does with the tables equals the thresholded member counts, at the planner's window and at windows of
    2 and 6 words (a destination of many windows, the last one ragged).  The all-ones row over neighbouring groups of exactly 255
    members is the carry case: every field at its maximum, an add more would run into the neighbour."""
    rng = np.random.default_rng(n + 5)
    bits = (rng.random((3, n)) < np.array([[0.5], [1.0], [0.03]])).astype(np.uint8)
    stride = max(16, ((n + 63) // 64 + 15) // 16 * 16) * 8
    rows = junk_rows(bits, stride)
    seen = set()
    for label, group_of, groups in collapse_maps(n) + [("runs255",) + runs_of_255(n)]:
        for which, need in need_vectors(group_of, groups):
            for window in (0, 2, 6):
                p = plan(plan_lib, n, group_of, groups, need, window=window)
                seen.add(p["field_bits"])
                want = consensus_rows(bits, group_of, groups, need, (p["dst_words"] + 1) // 2 * 16)
                for r in range(3):
                    assert np.array_equal(replay_kernel(plan_lib, p, rows[r]), want[r]), (n, label, which, window, r)
        if label == "runs255" and n >= 510:          # the carry case is really in it
            assert p["field_bits"] == 8 and p["largest"] == 255 and int(member_counts(bits, group_of, groups)[1, :2].min()) == 255
    assert seen == ({8, 16} if n > 255 else {8})


def test_replay_at_32_bit_fields(plan_lib):
    """One group of 65 536 members beside small ones: a field per LDS word.  The all-ones row, at the planner's window and at 2 words."""
    rng = np.random.default_rng(17)
    big, n, groups = 65_536, 65_536 + 700, 301
    group_of = np.concatenate([np.full(big, 150, np.uint32), rng.integers(0, groups, 700).astype(np.uint32)])
    group_of = group_of[rng.permutation(n)]
    bits = (rng.random((2, n)) < np.array([[1.0], [0.5]])).astype(np.uint8)
    rows = junk_rows(bits, ((n + 63) // 64 + 15) // 16 * 16 * 8)
    for which, need in need_vectors(group_of, groups):
        for window in (0, 2):
            p = plan(plan_lib, n, group_of, groups, need, window=window)
            assert p["field_bits"] == 32 and p["largest"] >= big
            want = consensus_rows(bits, group_of, groups, need, (p["dst_words"] + 1) // 2 * 16)
            for r in range(2):
                assert np.array_equal(replay_kernel(plan_lib, p, rows[r]), want[r]), (which, window, r)


def test_window_and_lds_invariants(plan_lib):
    k = constants(plan_lib)
    assert k["dropped"] == DROPPED and k["never"] == NEVER and k["window_words"] % 64 == 0
    assert k["window_words"] * 8 * (k["block"] // 64) <= k["lds_bytes"] <= 160 * 1024
    rng = np.random.default_rng(12)
    w64 = k["window_words"] * 64 // 8                                     # groups per window at 8-bit fields
    shapes = [(int(rng.integers(0, 100_000)), int(rng.integers(1, 5 * w64)), int(rng.integers(1, 20_000)), int(rng.choice([0, 1, 255, 256, 65_535, 65_536])))
              for _ in range(600)]
    shapes += [(70_000, g, 10_000_000, big) for big in (255, 256, 65_536) for g in (w64 * 8 // f + d for f in (8, 16, 32) for d in (-1, 0, 1))]
    shapes += [(100_000, g, 10_000_000, 100) for g in (1, 2, 63, 64, 65, 127, 128, 129)]
    shapes += [(5, g, m, 5) for g in (1, 100, 3 * w64 + 5) for m in (1, 2, 3, 4, 5, 4099)]
    first, count = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    for n, groups, m, big in shapes:
        big = min(big, n)
        group_of = np.full(max(n, 1), DROPPED, np.uint32)
        group_of[:big] = groups - 1                                       # one group of `big` members decides the field width
        p = plan(plan_lib, n, group_of, groups, m=m, tables=False)
        fb, waves_per_block = p["field_bits"], p["block"] // 64
        assert fb == (8 if big <= 255 else 16 if big <= 65_535 else 32) and p["largest"] == big
        assert p["window_words"] == k["window_words"] // fb and p["window_words"] % 2 == 0
        assert p["windows"] == max(1, -(-p["dst_words"] // p["window_words"]))
        assert p["image_words"] == min(p["window_words"], (max(p["dst_words"], 1) + 1) // 2 * 2) * fb
        assert p["image_words"] % (2 * fb) == 0 and 2 * fb <= p["image_words"] <= k["window_words"]
        assert p["lds_bytes"] == p["image_words"] * 8 * waves_per_block <= k["lds_bytes"]
        assert p["block"] % 64 == 0 and 1 <= waves_per_block <= k["block"] // 64 and waves_per_block <= max(m, 1)
        assert 1 <= p["grid"] and p["grid"] * waves_per_block <= k["waves"] and (p["grid"] - 1) * waves_per_block < max(m, 1)
        # the windows tile [0, dst_words) without gap or overlap, and each fits the image
        at = 0
        for j in range(p["windows"]):
            plan_lib.consensus_host_window(p["dst_words"], p["window_words"], j, ptr(first), ptr(count))
            assert int(first[0]) == at and 1 <= int(count[0]) <= p["window_words"] and (int(count[0]) + 1) // 2 * 2 * fb <= p["image_words"]
            at += int(count[0])
        assert at == p["dst_words"]
        plan_lib.consensus_host_window(p["dst_words"], p["window_words"], p["windows"], ptr(first), ptr(count))
        assert int(count[0]) == 0
    # 100 000 samples into 1000 random groups: one window of 8-bit fields
    group_of = np.random.default_rng(0).integers(0, 1000, 100_000).astype(np.uint32)
    p = plan(plan_lib, 100_000, group_of, 1000, m=10_000_000, tables=False)
    assert (p["windows"], p["field_bits"]) == (1, 8) and p["largest"] <= 255
    assert plan(plan_lib, 100_000, group_of, w64 + 1, tables=False)["windows"] == 2


def test_launch_shape(plan_lib):
    g = np.zeros(100, np.uint32)
    for m, block, grid in ((1, 64, 1), (2, 128, 1), (3, 192, 1), (4, 256, 1), (5, 256, 2), (4099, 256, 1024), (4096, 256, 1024), (10_000_000, 256, 1024)):
        p = plan(plan_lib, 100, g, 1, m=m, tables=False)
        assert (p["block"], p["grid"]) == (block, grid), m


# --------------------------------------------------------------------------------------------- percent -> members
def test_need_of():
    from bigsi_amd.consensus import group_sizes as sizes_of, member_counts as as_counts, need_of
    sizes = np.array([1, 2, 3, 10, 20, 100, 101, 255, 70_000], np.uint32)
    assert need_of(sizes, 100).dtype == np.uint32 and np.array_equal(need_of(sizes, 100), sizes)
    assert np.array_equal(need_of(np.arange(1, 101), 1), np.ones(100, np.uint32)) and need_of([101], 1).tolist() == [2]
    assert need_of([20], 95).tolist() == [19] and need_of([10], 10).tolist() == [1] and need_of([3], 50).tolist() == [2]
    assert need_of([0, 0], 100).tolist() == [1, 1] and need_of([], 50).size == 0          # a group without members needs 1 (and stays zero)
    assert need_of([0xFFFFFFFE], 100).tolist() == [0xFFFFFFFE] and need_of([7], np.int64(100)).tolist() == [7]
    for s in (1, 7, 99, 100, 101, 12_345):                                 # need = ceil(percent x size / 100), at least 1
        for pc in (1, 33, 50, 67, 99, 100):
            assert need_of([s], pc).tolist() == [max(1, -(-pc * s // 100))]
    for bad in (True, False, 50.0, "50", None, np.float32(3)):
        with pytest.raises(TypeError):
            need_of(sizes, bad)
    for bad in (0, 101, -1, 1000):
        with pytest.raises(ValueError):
            need_of(sizes, bad)
    for bad in (np.array([1.5]), np.array([-1]), np.array([1 << 32]), np.ones((2, 2), np.uint32)):
        with pytest.raises(ValueError):
            need_of(bad, 50)
    g = np.array([0, 2, DROPPED, 2, 0, 2], np.uint32)
    assert sizes_of(g, 4).tolist() == [2, 0, 3, 0] and sizes_of(g, 4).dtype == np.uint32
    need = np.array([1, 5, NEVER], np.uint32)
    assert np.array_equal(as_counts(need, 3), need) and as_counts([1, 5, NEVER], 3).dtype == np.uint32
    for bad, groups in ((need[:2], 3), (need.astype(np.float64), 3), (np.array([1, -1, 1]), 3), (np.array([1, 1 << 32, 1]), 3), (np.array([1, 0, 1]), 3),
                        (need.reshape(3, 1), 3)):
        with pytest.raises(ValueError):
            as_counts(bad, groups)


# --------------------------------------------------------------------------------------------- decided before any device call
def test_consensus_checks_its_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    cfg = {"m": 1, "h": 1, "k": 1}
    for groups, keep, err in (({}, False, ValueError), ([], False, ValueError), ({"A": []}, False, ValueError), ({"A": ["x"], "B": ["x"]}, False, ValueError),
                              ({DELETED: ["x"]}, False, ValueError), ("abc", False, TypeError), ({"A": "x"}, False, TypeError), ({"A": ["x"]}, "yes", TypeError)):
        with pytest.raises(err):
            b.consensus(cfg, groups, keep_others=keep)
    for percent, err in ((0, ValueError), (101, ValueError), (-5, ValueError), (True, TypeError), (99.0, TypeError), ("60", TypeError), (None, TypeError)):
        with pytest.raises(err):
            b.consensus(cfg, {"A": ["x"]}, percent=percent)


def test_abi_lists_the_new_entry_point():
    from bigsi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_consensus.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.CONSENSUS_SIGNATURES) == ["bigsi_hip_consensus_columns_into"]
    name = declared[0]
    assert getattr(_lib.lib(), name).argtypes == _lib.CONSENSUS_SIGNATURES[name][1] and len(_lib.CONSENSUS_SIGNATURES[name][1]) == 5
    assert _lib.CONSENSUS_SIGNATURES[name][1][3] is C.c_uint64 and _lib.CONSENSUS_SIGNATURES[name][0] is C.c_int32
    assert all(name not in t for t in (_lib.SIGNATURES, _lib.COMPACT_SIGNATURES, _lib.FOLD_SIGNATURES, _lib.PREVALENCE_SIGNATURES, _lib.COLLAPSE_SIGNATURES,
                                       _lib.PAIRWISE_SIGNATURES))
    assert sorted(_lib.COLLAPSE_SIGNATURES) == ["bigsi_hip_collapse_columns_into"]          # the collapse's header and table keep their one name
    header = open(os.path.join(ROOT, "include", "bigsi_cpu_consensus.h")).read()
    assert "#define bigsi_hip_consensus_columns_into bigsi_cpu_consensus_columns_into" in header and "BIGSI_USE_CPU_TWIN" in header
    for other in ("bigsi_hip.h", "bigsi_hip_collapse.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert name not in re.sub(r"/\*.*?\*/", "", text, flags=re.S), other


def test_cli_parsing():
    from bigsi_amd.__main__ import build_parser
    p = build_parser()[0]
    a = p.parse_args(["consensus", "to.yaml", "--groups", "g.tsv", "-c", "c.yaml"])
    assert (a.cmd, a.to_config, a.groups, a.percent, a.keep_others, a.config) == ("consensus", "to.yaml", "g.tsv", 100, False, "c.yaml")
    a = p.parse_args(["consensus", "to.yaml", "--groups", "g.tsv", "--percent", "60", "--keep-others"])
    assert (a.percent, a.keep_others) == (60, True)
    for argv in (["consensus", "to.yaml"], ["consensus", "--groups", "g.tsv"], ["consensus", "to.yaml", "--groups", "g.tsv", "--percent", "60.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    p.format_help()                                                       # (a stray % in a help text would raise here)


def test_cli_refuses_sharded(capsys):
    from bigsi_amd.__main__ import main
    with pytest.raises(SystemExit):
        main(["consensus", "to.yaml", "--groups", "g.tsv", "--sharded"])
    err = capsys.readouterr().err
    assert "--sharded" in err and "consensus" in err


class _FakeIndex(object):
    def __init__(self, names):
        self.names, self.num_samples, self.asked = names, len(names), None

    def colour_to_sample(self, c):
        return self.names[c]

    def consensus(self, config, groups, percent=100, keep_others=False):
        self.asked = (config, groups, percent, keep_others)
        return _FakeIndex(["g"] * (3 if keep_others else 2))


def test_cli_consensus_text(tmp_path):
    import yaml
    from bigsi_amd.__main__ import consensus_text
    to = tmp_path / "to.yaml"
    to.write_text(yaml.safe_dump({"k": 3, "m": 10, "h": 1, "storage-engine": "hip-hbm", "storage-config": {"name": "x"}}))
    ix = _FakeIndex(["s0", "s1", DELETED, "s3", "s4", "s5"])
    pairs = [("s4", "B"), ("s0", "A"), ("s1", "B"), ("s5", "B")]
    out = json.loads(consensus_text(ix, "c.yaml", str(to), pairs, percent=60))
    assert out == {"result": "consensus of 4 of 5 samples from c.yaml at 60 %% into 2 groups in %s." % to, "groups": 2, "samples_in": 5, "samples_dropped": 1,
                   "num_samples": 2, "members": {"B": ["s1", "s4", "s5"], "A": ["s0"]}, "percent": 60, "min_members": {"B": 2, "A": 1}}
    assert ix.asked[1] == pairs and ix.asked[2] == 60 and ix.asked[3] is False and ix.asked[0]["m"] == 10
    out = json.loads(consensus_text(ix, "c.yaml", str(to), pairs, keep_others=True))
    assert (out["groups"], out["samples_dropped"], out["members"]["s3"], out["percent"]) == (3, 0, ["s3"], 100)
    assert out["min_members"] == {"B": 3, "A": 1, "s3": 1}               # a sample kept on its own needs 1: it is copied


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planner_and_twin(tmp_path):
    """tests/c_host/consensus_sanitize_main.cpp -- a program with its own main that drives plan_consensus_columns, the kernel's
    arithmetic replayed from its tables and the twin's bigsi_cpu_consensus_columns_into over odd shapes -- built with AddressSanitizer
    and UndefinedBehaviorSanitizer and run as a process of its own."""
    exe = str(tmp_path / "consensus_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "consensus_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "consensus planner and twin: ok", (r.stdout[-1000:], r.stderr[-3000:])
