"""Column collapse without a GPU: the CPU twin of bigsi_hip_collapse_columns_into against numpy on the very bits written
(expected[:, g] = bits[:, group_of == g].any(axis=1), packed, zero to the stride), the per-call tables of plan_collapse_columns
(csrc/bigsi_launch.hpp, compiled by g++) against a bit-by-bit restatement of the row format -- and the kernel's own arithmetic replayed
from those tables --, the window and LDS invariants of the planner, the derivation of group maps from name lists
(bigsi_amd/collapse.py), what BIGSI.collapse and its command line decide before any device call, and a stand-alone sanitized program
over the planner and the twin."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raw_index import ptr, ragged_bits
from test_compact_columns_host import WIDTHS, Info, pack_keep

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_STATE = -1, -6
DROPPED = 0xFFFFFFFF
DELETED = "D3L3T3D"


def collapse_maps(n, seed=0):
    """[(label, group_of uint32[n], G)]: the maps every width is collapsed with."""
    rng = np.random.default_rng(2000 + n + seed)
    ar = np.arange(n, dtype=np.uint32)
    maps = [("identity", ar.copy(), n), ("reversal", (n - 1 - ar).astype(np.uint32), n), ("permutation", rng.permutation(n).astype(np.uint32), n),
            ("one", np.zeros(n, np.uint32), 1)]
    g = max(1, n // 3)
    many = rng.integers(0, g, n).astype(np.uint32)
    many[rng.random(n) < 0.2] = DROPPED
    maps.append(("many", many, g))
    g = max(4, n // 2 + 3)                                                # groups 0, g // 2 and g - 1 stay without members
    allowed = np.setdiff1d(np.arange(g), [0, g // 2, g - 1])
    maps.append(("emptygroups", allowed[rng.integers(0, allowed.size, n)].astype(np.uint32), g))
    only = np.full(n, DROPPED, np.uint32)
    only[n // 2] = 2
    maps.append(("onlyone", only, 3))
    flags = rng.random(n) < 0.5
    flags[n - 1] = True
    inj = np.full(n, DROPPED, np.uint32)
    inj[flags] = np.arange(int(flags.sum()), dtype=np.uint32)
    maps.append(("monotone", inj, int(flags.sum())))
    return maps


def expected_rows(bits, group_of, groups, row_bytes):
    """numpy on the very bits written: column g = the OR of the columns of group g, packed, zero up to row_bytes."""
    exp = np.zeros((groups, bits.shape[0]), np.uint8)
    cols = np.flatnonzero(group_of != DROPPED)
    np.maximum.at(exp, group_of[cols].astype(np.int64), bits[:, cols].T)
    want = np.zeros((bits.shape[0], row_bytes), np.uint8)
    packed = np.packbits(exp.T, axis=1)
    want[:, :packed.shape[1]] = packed
    return want


def junk_rows(bits, stride, seed=1):
    """The rows of `bits` at the full stride, every bit behind the last column set at random: none of it may survive."""
    m, n = bits.shape
    rng = np.random.default_rng(seed)
    full = (rng.random((m, stride * 8)) < 0.5).astype(np.uint8)
    full[:, :n] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1))


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    L.bigsi_cpu_collapse_columns_into.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.bigsi_cpu_collapse_columns_into.restype = C.c_int32
    return L


def twin_open(L, m, n, cap=None, h=3):
    ix = C.c_void_p()
    assert L.bigsi_cpu_open(C.c_uint64(m), C.c_uint64(n), C.c_uint64(cap or n), C.c_uint32(h), 0, C.byref(ix)) == 0
    return ix


def twin_info(L, ix):
    inf = Info()
    assert L.bigsi_cpu_get_info(ix, C.byref(inf)) == 0
    return inf


def twin_write(L, ix, packed):
    ids = np.arange(packed.shape[0], dtype=np.uint64)
    assert L.bigsi_cpu_set_rows(ix, ptr(ids), C.c_uint64(ids.size), ptr(packed), C.c_uint64(packed.shape[1])) == 0, L.bigsi_cpu_last_error()


def twin_rows(L, ix, m, row_bytes):
    out = np.full((m, row_bytes), 0xAB, np.uint8)
    ids = np.arange(m, dtype=np.uint64)
    assert L.bigsi_cpu_get_rows(ix, ptr(ids), C.c_uint64(m), ptr(out), C.c_uint64(row_bytes)) == 0, L.bigsi_cpu_last_error()
    return out


def twin_source(L, bits):
    """A twin index holding `bits`, with junk behind the last column up to the stride; returns (handle, the bytes written)."""
    m, n = bits.shape
    ix = twin_open(L, m, n)
    packed = junk_rows(bits, int(twin_info(L, ix).row_stride_bytes))
    twin_write(L, ix, packed)
    return ix, packed


@pytest.mark.parametrize("n", WIDTHS)
def test_twin_against_numpy(cpu, n):
    m = 257 if n < 1000 else 41
    bits = ragged_bits(m, n)
    for label, group_of, groups in collapse_maps(n):
        src, written = twin_source(cpu, bits)
        dst = twin_open(cpu, m, 0, 1)
        assert cpu.bigsi_cpu_collapse_columns_into(dst, src, ptr(group_of), groups) == 0, cpu.bigsi_cpu_last_error()
        info = twin_info(cpu, dst)
        assert info.num_cols == groups and info.col_capacity >= groups, (n, label)
        for rb in ((groups + 7) // 8, int(info.row_stride_bytes)):          # the stride padding is zero, no junk came along
            assert np.array_equal(twin_rows(cpu, dst, m, rb), expected_rows(bits, group_of, groups, rb)), (n, label, rb)
        assert np.array_equal(twin_rows(cpu, src, m, written.shape[1]), written) and twin_info(cpu, src).num_cols == n          # only read
        if label == "identity":
            assert np.array_equal(twin_rows(cpu, dst, m, (n + 7) // 8), np.packbits(bits, axis=1))
        if label == "monotone":          # = the extraction of the same columns
            flags = group_of != DROPPED
            ext = twin_open(cpu, m, 0, 1)
            assert cpu.bigsi_cpu_extract_columns(ext, src, ptr(pack_keep(flags))) == 0, cpu.bigsi_cpu_last_error()
            rb = int(min(info.row_stride_bytes, twin_info(cpu, ext).row_stride_bytes))
            assert np.array_equal(twin_rows(cpu, dst, m, rb), twin_rows(cpu, ext, m, rb))
            assert cpu.bigsi_cpu_close(ext) == 0
        for h in (src, dst):
            assert cpu.bigsi_cpu_close(h) == 0


def test_twin_refusals(cpu):
    bits = ragged_bits(64, 100)
    g = (np.arange(100) % 7).astype(np.uint32)
    src, _ = twin_source(cpu, bits)
    full, _ = twin_source(cpu, bits)
    other_m, other_h, empty = twin_open(cpu, 65, 0, 1), twin_open(cpu, 64, 0, 1, h=2), twin_open(cpu, 64, 0, 1)
    bad = g.copy()
    bad[41] = 7
    call = cpu.bigsi_cpu_collapse_columns_into
    for args, want, words in (((None, src, ptr(g), 7), ERR_INVALID, ()),
                              ((empty, None, ptr(g), 7), ERR_INVALID, ()),
                              ((empty, src, None, 7), ERR_INVALID, ()),
                              ((empty, src, ptr(g), 0), ERR_INVALID, ("0",)),
                              ((empty, src, ptr(g), 0xFFFFFFFF), ERR_INVALID, ("4294967295",)),
                              ((empty, src, ptr(g), 1 << 40), ERR_INVALID, ()),
                              ((empty, src, ptr(bad), 7), ERR_INVALID, ("41", "7")),          # the message names the column and the value
                              ((src, src, ptr(g), 7), ERR_INVALID, ()),                       # dst == src
                              ((other_m, src, ptr(g), 7), ERR_INVALID, ("65", "64")),
                              ((other_h, src, ptr(g), 7), ERR_INVALID, ("2", "3")),
                              ((full, src, ptr(g), 7), ERR_STATE, ("100",))):                 # a destination that holds columns
        rc = call(*args)
        msg = cpu.bigsi_cpu_last_error().decode()
        assert rc == want and msg and all(w in msg for w in words), (rc, want, msg)
    for h in (empty, other_m, other_h):          # a refused call left the destination empty
        assert twin_info(cpu, h).num_cols == 0 and not twin_rows(cpu, h, 64, int(twin_info(cpu, h).row_stride_bytes)).any()
    assert twin_info(cpu, full).num_cols == 100
    sentinel_ok = g.copy()
    sentinel_ok[41] = DROPPED                    # ... and the sentinel is no bad entry
    assert call(empty, src, ptr(sentinel_ok), 7) == 0 and twin_info(cpu, empty).num_cols == 7
    for h in (src, full, other_m, other_h, empty):
        assert cpu.bigsi_cpu_close(h) == 0


# --------------------------------------------------------------------------------------------- the plan's tables
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("collapse_host") / "libcollapse_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "collapse_host.cpp")])
    lib = C.CDLL(so)
    lib.collapse_host_first_bad.restype = C.c_uint64
    lib.collapse_host_mem_bit.restype = C.c_uint32
    lib.collapse_host_plan.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.collapse_host_window.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


HEAD = ("src_words", "table_words", "dst_words", "window_words", "windows", "image_words", "block", "grid", "lds_bytes", "moved")
CONSTS = ("dropped", "waves", "window_words", "lds_bytes", "loads", "gathers", "block")


def constants(lib):
    c = np.zeros(7, np.uint64)
    lib.collapse_host_constants(ptr(c))
    return dict(zip(CONSTS, (int(x) for x in c)))


def plan(lib, n, group_of, groups, m=1000, window=0, tables=True):
    tw = ((n + 63) // 64 + 1) // 2 * 2
    head = np.zeros(10, np.uint64)
    dst_bit, live = np.zeros(max(tw * 64, 1), np.uint32), np.zeros(max(tw, 1), np.uint64)
    rc = lib.collapse_host_plan(n, ptr(group_of), groups, m, window, ptr(head), ptr(dst_bit) if tables else None, tw * 64, ptr(live) if tables else None, tw)
    assert rc == 0
    p = dict(zip(HEAD, (int(x) for x in head)))
    assert p["src_words"] == (n + 63) // 64 and p["table_words"] == tw and p["dst_words"] == (groups + 63) // 64
    p["dst_bit"], p["live"] = dst_bit[:tw * 64], live[:tw]
    return p


def mem_bit(c):
    """Where column c of a 64-column word lies in the little-endian 64-bit word as it is in memory: byte c // 8 under mask 0x80 >> c % 8."""
    return 8 * (c // 8) + 7 - c % 8


def test_mem_bit_is_the_row_format(plan_lib):
    for c in range(64):
        word = np.zeros(8, np.uint8)
        word[c // 8] = 0x80 >> (c % 8)                                   # the row format's byte and mask of column c
        assert int(word.view("<u8")[0]) == 1 << plan_lib.collapse_host_mem_bit(c) == 1 << mem_bit(c)
        assert plan_lib.collapse_host_mem_bit(plan_lib.collapse_host_mem_bit(c)) == c          # its own inverse


@pytest.mark.parametrize("n", WIDTHS)
def test_plan_tables_against_restatement(plan_lib, n):
    for label, group_of, groups in collapse_maps(n):
        p = plan(plan_lib, n, group_of, groups)
        want_bit, want_live = np.full(p["table_words"] * 64, DROPPED, np.uint32), [0] * p["table_words"]
        for c in range(n):
            g = int(group_of[c])
            if g == DROPPED:
                continue
            want_bit[64 * (c // 64) + mem_bit(c % 64)] = 64 * (g // 64) + mem_bit(g % 64)
            want_live[c // 64] |= 1 << mem_bit(c % 64)
        assert np.array_equal(p["dst_bit"], want_bit), (n, label)
        assert [int(x) for x in p["live"]] == want_live, (n, label)
        assert p["moved"] == int((group_of != DROPPED).sum())
        # live is exactly the set of bits with a table entry (the kernel tests live, never the sentinel)
        live_bits = np.unpackbits(p["live"].view(np.uint8), bitorder="little")
        assert np.array_equal(live_bits.astype(bool), p["dst_bit"] != DROPPED)
        assert plan_lib.collapse_host_first_bad(n, ptr(group_of), groups) == n
    bad = np.zeros(n, np.uint32)
    bad[n // 2] = 5
    assert plan_lib.collapse_host_first_bad(n, ptr(bad), 5) == n // 2


def replay_kernel(lib, p, src_row):
    """k_collapse_columns' walk over one row from the tables: the set bits of (source & live) by their memory bit address, their
    dst_bit entries, window by window the ones inside [lo, lo + span) ORed into an image of image_words words, the image read out in
    pairs of words and cleared.  Returns the destination row's bytes up to round_up(dst_words, 2) words."""
    tw, dw = p["table_words"], p["dst_words"]
    src_bits = np.unpackbits(src_row[:tw * 8], bitorder="little")         # index = bit address in memory
    live_bits = np.unpackbits(p["live"].view(np.uint8), bitorder="little")
    addrs = p["dst_bit"][np.flatnonzero(src_bits & live_bits)].astype(np.int64)
    out = np.zeros((dw + 1) // 2 * 2 * 64, np.uint8)
    image = np.zeros(p["image_words"] * 64, np.uint8)
    first, count = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    for j in range(p["windows"]):
        lib.collapse_host_window(dw * 64, p["window_words"], j, ptr(first), ptr(count))
        lo, span = int(first[0]) * 64, int(count[0]) * 64
        rel = (addrs - lo) % (1 << 32)                                    # (the kernel's 32-bit wrap)
        image[rel[rel < span]] = 1
        pairs = (int(count[0]) + 1) // 2 * 2 * 64
        assert pairs <= image.size
        out[lo:lo + pairs] = image[:pairs]
        image[:pairs] = 0
    assert not image.any()
    return np.packbits(out, bitorder="little")


@pytest.mark.parametrize("n", (1, 64, 65, 129, 1025, 8193))
def test_kernel_arithmetic_replayed_from_the_tables(plan_lib, n):
    """What k_collapse_columns does with the tables equals the OR of the columns of every group, at the planner's window and at
    windows of 2 and 6 words (a destination of many windows, the last one ragged)."""
    rng = np.random.default_rng(n + 5)
    bits = (rng.random((3, n)) < np.array([[0.5], [1.0], [0.03]])).astype(np.uint8)
    stride = max(16, ((n + 63) // 64 + 15) // 16 * 16) * 8
    rows = junk_rows(bits, stride)
    for label, group_of, groups in collapse_maps(n):
        for window in (0, 2, 6):
            p = plan(plan_lib, n, group_of, groups, window=window)
            want = expected_rows(bits, group_of, groups, (p["dst_words"] + 1) // 2 * 16)
            for r in range(3):
                assert np.array_equal(replay_kernel(plan_lib, p, rows[r]), want[r]), (n, label, window, r)


def test_window_and_lds_invariants(plan_lib):
    k = constants(plan_lib)
    assert k["dropped"] == DROPPED and k["window_words"] % 2 == 0 and k["window_words"] * 8 * (k["block"] // 64) <= k["lds_bytes"] <= 160 * 1024
    w64 = k["window_words"] * 64
    rng = np.random.default_rng(11)
    shapes = [(int(rng.integers(0, 200_000)), int(rng.integers(1, 5 * w64)), int(rng.integers(1, 20_000))) for _ in range(3000)]
    shapes += [(100_000, g, 10_000_000) for g in (w64 - 1, w64, w64 + 1, 2 * w64 - 1, 2 * w64, 2 * w64 + 1, 1, 2, 63, 64, 65, 127, 128, 129)]
    shapes += [(5, g, m) for g in (1, 100, 3 * w64 + 5) for m in (1, 2, 3, 4, 5, 4099)]
    dropped = np.full(200_000, DROPPED, np.uint32)
    first, count = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    for n, groups, m in shapes:
        p = plan(plan_lib, n, dropped, groups, m=m, tables=False)
        waves_per_block = p["block"] // 64
        assert p["window_words"] == k["window_words"] and p["windows"] == max(1, -(-p["dst_words"] // p["window_words"]))
        assert p["image_words"] % 2 == 0 and 2 <= p["image_words"] <= p["window_words"]
        assert p["lds_bytes"] == p["image_words"] * 8 * waves_per_block <= k["lds_bytes"]
        assert p["block"] % 64 == 0 and 1 <= waves_per_block <= k["block"] // 64 and waves_per_block <= max(m, 1)
        assert 1 <= p["grid"] and p["grid"] * waves_per_block <= k["waves"] and (p["grid"] - 1) * waves_per_block < max(m, 1)
        # the windows tile [0, dst_words) without gap or overlap, and each fits the image
        at = 0
        for j in range(p["windows"]):
            plan_lib.collapse_host_window(groups, 0, j, ptr(first), ptr(count))
            assert int(first[0]) == at and 1 <= int(count[0]) <= p["window_words"] and (int(count[0]) + 1) // 2 * 2 <= p["image_words"]
            at += int(count[0])
        assert at == p["dst_words"]
        plan_lib.collapse_host_window(groups, 0, p["windows"], ptr(first), ptr(count))
        assert int(count[0]) == 0
    # one window for the 100 k-sample index
    assert plan(plan_lib, 100_000, dropped, 100_000, m=10_000_000, tables=False)["windows"] == 1
    assert plan(plan_lib, 100_000, dropped, w64 + 1, tables=False)["windows"] == 2


def test_launch_shape(plan_lib):
    g = np.zeros(100, np.uint32)
    for m, block, grid in ((1, 64, 1), (2, 128, 1), (3, 192, 1), (4, 256, 1), (5, 256, 2), (4099, 256, 1024), (4096, 256, 1024), (10_000_000, 256, 1024)):
        p = plan(plan_lib, 100, g, 1, m)
        assert (p["block"], p["grid"]) == (block, grid), m


# --------------------------------------------------------------------------------------------- name lists -> group maps
def test_collapse_plan_on_hand_made_names():
    from bigsi_amd.collapse import DROPPED as D, collapse_plan
    assert D == DROPPED
    names = ["s%d" % c for c in range(70)]
    names[5] = DELETED
    groups = {"B": ["s69", "s0"], "A": ["s64"], "C": ["s63", "s1", "s2"]}
    group_of, out, members = collapse_plan(names, groups)
    want = np.full(70, DROPPED, np.uint32)
    want[[69, 0]], want[64], want[[63, 1, 2]] = 0, 1, 2
    assert group_of.dtype == np.uint32 and np.array_equal(group_of, want)
    assert out == ["B", "A", "C"] and members == [["s0", "s69"], ["s64"], ["s1", "s2", "s63"]]          # first appearance; members in colour order
    # the same as pairs, in any order of the samples: the colour of a group follows its first pair
    pairs = [("s69", "B"), ("s64", "A"), ("s63", "C"), ("s0", "B"), ("s1", "C"), ("s2", "C")]
    g2, out2, members2 = collapse_plan(names, pairs)
    assert np.array_equal(g2, want) and out2 == out and members2 == members
    # keep_others: every unlisted live sample a group of its own, after the named groups, in colour order; deleted ones dropped
    g3, out3, members3 = collapse_plan(names, groups, keep_others=True)
    rest = [n for c, n in enumerate(names) if n != DELETED and want[c] == DROPPED]
    assert out3 == out + rest and members3 == members + [[n] for n in rest]
    assert g3[5] == DROPPED and int((g3 == DROPPED).sum()) == 1 and sorted(g3[g3 != DROPPED].tolist()) == sorted([0, 0, 1, 2, 2, 2] + list(range(3, 3 + len(rest))))
    assert [int(g3[names.index(n)]) for n in rest] == list(range(3, 3 + len(rest)))
    # an injective map reorders
    g4, out4, _ = collapse_plan(["a", "b", "c"], [("c", "c"), ("a", "a"), ("b", "b")])
    assert g4.tolist() == [1, 2, 0] and out4 == ["c", "a", "b"]


def test_collapse_plan_errors():
    from bigsi_amd.collapse import collapse_plan
    names = ["s0", "s1", DELETED, "s3"]
    for groups, keep, err in (({"A": ["nobody"]}, False, KeyError),
                              ({"A": [DELETED]}, False, KeyError),
                              ({"A": ["s0"], "B": ["s0"]}, False, ValueError),          # a sample in two groups
                              ([("s0", "A"), ("s1", "B"), ("s0", "B")], False, ValueError),
                              ({"A": ["s0", "s0"]}, False, ValueError),
                              ({"A": ["s0"], "B": []}, False, ValueError),             # an empty group
                              ({}, False, ValueError),                                 # no groups
                              ([], False, ValueError),
                              ({DELETED: ["s0"]}, False, ValueError),
                              ({"s3": ["s0", "s1"]}, True, ValueError),                # with keep_others: the name of a kept sample
                              ("s0", False, TypeError),
                              ({"A": "s0"}, False, TypeError),
                              ({"A": ["s0"]}, 1, TypeError)):
        with pytest.raises(err):
            collapse_plan(names, groups, keep)
    # ... which is fine when that sample is a member, or dropped
    assert collapse_plan(names, {"s3": ["s0", "s3"]}, True)[1] == ["s3", "s1"]
    assert collapse_plan(names, {"s3": ["s0", "s1"]}, False)[1] == ["s3"]


def test_group_ids_validation():
    from bigsi_amd.collapse import group_ids
    g = np.array([0, 2, DROPPED, 1], np.uint32)
    assert np.array_equal(group_ids(g, 4, 3), g) and group_ids(g.astype(np.int64), 4, 3).dtype == np.uint32
    assert np.array_equal(group_ids([0, 2, DROPPED, 1], 4, 3), g)
    for bad, n, groups in ((g[:3], 4, 3), (g.astype(np.float64), 4, 3), (np.array([0, -1, 0, 0]), 4, 3), (np.array([0, 1 << 32, 0, 0]), 4, 3), (g, 4, 0),
                           (g, 4, DROPPED), (g.reshape(2, 2), 4, 3)):
        with pytest.raises(ValueError):
            group_ids(bad, n, groups)


# --------------------------------------------------------------------------------------------- decided before any device call
def test_collapse_checks_its_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    cfg = {"m": 1, "h": 1, "k": 1}
    for groups, keep, err in (({}, False, ValueError), ([], False, ValueError), ({"A": []}, False, ValueError), ({"A": ["x"], "B": ["x"]}, False, ValueError),
                              ({DELETED: ["x"]}, False, ValueError), ("abc", False, TypeError), ({"A": "x"}, False, TypeError), ({"A": ["x"]}, "yes", TypeError)):
        with pytest.raises(err):
            b.collapse(cfg, groups, keep_others=keep)


def test_abi_lists_the_new_entry_point():
    from bigsi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_collapse.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.COLLAPSE_SIGNATURES) == ["bigsi_hip_collapse_columns_into"]
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.COLLAPSE_SIGNATURES[name][1]
        assert all(name not in t for t in (_lib.SIGNATURES, _lib.COMPACT_SIGNATURES, _lib.FOLD_SIGNATURES, _lib.PREVALENCE_SIGNATURES))
    assert "0xFFFFFFFFu" in src and _lib.COLLAPSE_SIGNATURES["bigsi_hip_collapse_columns_into"][1][3] is C.c_uint64
    header = open(os.path.join(ROOT, "include", "bigsi_cpu_collapse.h")).read()
    assert "#define bigsi_hip_collapse_columns_into bigsi_cpu_collapse_columns_into" in header
    hip_h = open(os.path.join(ROOT, "include", "bigsi_hip.h")).read()
    assert "bigsi_hip_collapse_columns_into" not in re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S)          # bigsi_hip.h keeps its entry points


def test_cli_parsing_and_groups_file(tmp_path):
    from bigsi_amd.__main__ import build_parser, collapse_groups
    p = build_parser()[0]
    a = p.parse_args(["collapse", "to.yaml", "--groups", "g.tsv", "-c", "c.yaml"])
    assert (a.cmd, a.to_config, a.groups, a.keep_others, a.config) == ("collapse", "to.yaml", "g.tsv", False, "c.yaml")
    assert p.parse_args(["collapse", "to.yaml", "--groups", "g.tsv", "--keep-others"]).keep_others is True
    for argv in (["collapse", "to.yaml"], ["collapse", "--groups", "g.tsv"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    f = tmp_path / "g.tsv"
    f.write_text("s1\tA\n\ns0\tB \n s2\tA\r\n")
    assert collapse_groups(str(f)) == [("s1", "A"), ("s0", "B"), ("s2", "A")]
    for bad in ("s1 A\n", "s1\tA\tx\n", "s1\t\n", "\tA\n"):
        f.write_text("s0\tB\n" + bad)
        with pytest.raises(ValueError) as e:
            collapse_groups(str(f))
        assert "line 2" in str(e.value)


def test_cli_refuses_sharded(capsys):
    from bigsi_amd.__main__ import main
    with pytest.raises(SystemExit):
        main(["collapse", "to.yaml", "--groups", "g.tsv", "--sharded"])
    err = capsys.readouterr().err
    assert "--sharded" in err and "collapse" in err


class _FakeIndex(object):
    def __init__(self, names):
        self.names, self.num_samples, self.asked = names, len(names), None

    def colour_to_sample(self, c):
        return self.names[c]

    def collapse(self, config, groups, keep_others=False):
        self.asked = (config, groups, keep_others)
        return _FakeIndex(["g"] * (3 if keep_others else 2))


def test_cli_collapse_text(tmp_path):
    import yaml
    from bigsi_amd.__main__ import collapse_text
    to = tmp_path / "to.yaml"
    to.write_text(yaml.safe_dump({"k": 3, "m": 10, "h": 1, "storage-engine": "hip-hbm", "storage-config": {"name": "x"}}))
    ix = _FakeIndex(["s0", "s1", DELETED, "s3", "s4"])
    pairs = [("s4", "B"), ("s0", "A"), ("s1", "B")]
    out = json.loads(collapse_text(ix, "c.yaml", str(to), pairs))
    assert out == {"result": "collapsed 3 of 4 samples from c.yaml into 2 groups in %s." % to, "groups": 2, "samples_in": 4, "samples_dropped": 1,
                   "num_samples": 2, "members": {"B": ["s1", "s4"], "A": ["s0"]}}
    assert ix.asked[1] == pairs and ix.asked[2] is False and ix.asked[0]["m"] == 10
    out = json.loads(collapse_text(ix, "c.yaml", str(to), pairs, keep_others=True))
    assert (out["groups"], out["samples_dropped"], out["members"]["s3"]) == (3, 0, ["s3"])


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planner_and_twin(tmp_path):
    """tests/c_host/collapse_sanitize_main.cpp -- a program with its own main that drives plan_collapse_columns, the kernel's
    arithmetic replayed from its tables and the twin's bigsi_cpu_collapse_columns_into over odd shapes -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a process of its own."""
    exe = str(tmp_path / "collapse_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "collapse_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "collapse planner and twin: ok", (r.stdout[-1000:], r.stderr[-3000:])
