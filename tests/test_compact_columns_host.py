"""Column compaction without a GPU: the CPU twin of bigsi_hip_compact_columns / bigsi_hip_extract_columns against numpy on the rows
written, the per-call tables of plan_compact_columns (csrc/bigsi_launch.hpp, compiled by g++) against a bit-by-bit restatement --
and the kernel's own arithmetic replayed from those tables --, the derivation of keep bitmaps from name lists
(bigsi_amd/compact.py), and what vacuum / extract and their command lines decide before any device call."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raw_index import ptr, ragged_bits

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_STATE = -1, -6
WIDTHS = (1, 8, 63, 64, 65, 127, 128, 129, 1023, 1025, 8191, 8193)
DELETED = "D3L3T3D"


def pack_keep(flags, junk=False):
    """Column selector (bool[n]) in the row format; junk: every bit of the last byte past column n - 1 set."""
    by = np.packbits(np.asarray(flags, dtype=bool))
    if junk and flags.size % 8:
        by[-1] |= (1 << (8 - flags.size % 8)) - 1
    return np.ascontiguousarray(by) if by.size else np.zeros(1, np.uint8)


def keep_patterns(n, seed=0):
    """[(label, bool[n], keep bitmap)]: the selections every width is compacted with."""
    rng = np.random.default_rng(1000 + n + seed)
    every, none = np.ones(n, bool), np.zeros(n, bool)
    pats = [("all", every), ("none", none)]
    f = none.copy(); f[0] = True; pats.append(("only0", f))
    f = none.copy(); f[-1] = True; pats.append(("onlylast", f))
    f = every.copy(); f[0] = False; pats.append(("not0", f))
    f = every.copy(); f[-1] = False; pats.append(("notlast", f))
    f = none.copy(); f[::2] = True; pats.append(("alternate", f))
    w = min(1, (n - 1) // 64)
    f = every.copy(); f[64 * w:64 * w + 64] = False; pats.append(("wordgone", f))
    f = none.copy(); c = 64 * np.arange((n + 63) // 64) + (np.arange((n + 63) // 64) * 7) % 64; f[c[c < n]] = True; pats.append(("oneperword", f))
    f = none.copy(); f[(n - 1) // 64 * 64:] = rng.random(n - (n - 1) // 64 * 64) < 0.6; f[-1] = True; pats.append(("lastword", f))
    for d in (0.9, 0.5, 0.05):
        pats.append(("random%g" % d, rng.random(n) < d))
    out = [(label, f, pack_keep(f)) for label, f in pats]
    f = rng.random(n) < 0.5
    out.append(("junk", f, pack_keep(f, junk=True)))
    return out


def expected_rows(bits, flags, row_bytes):
    """numpy on the very bits written: the kept columns packed, zero up to row_bytes."""
    want = np.zeros((bits.shape[0], row_bytes), np.uint8)
    if flags.any():
        packed = np.packbits(bits[:, flags], axis=1)
        want[:, :packed.shape[1]] = packed
    return want


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    return L


class Info(C.Structure):
    _fields_ = [("num_rows", C.c_uint64), ("num_cols", C.c_uint64), ("col_capacity", C.c_uint64), ("row_bytes", C.c_uint64),
                ("row_stride_bytes", C.c_uint64), ("index_bytes", C.c_uint64), ("num_hashes", C.c_uint32), ("device", C.c_int32)]


def twin_open(L, m, n, cap=None):
    ix = C.c_void_p()
    assert L.bigsi_cpu_open(C.c_uint64(m), C.c_uint64(n), C.c_uint64(cap or n), C.c_uint32(3), 0, C.byref(ix)) == 0
    return ix


def twin_index(L, bits, cap=None):
    m, n = bits.shape
    ix = twin_open(L, m, n, cap)
    packed = np.ascontiguousarray(np.packbits(bits, axis=1))
    ids = np.arange(m, dtype=np.uint64)
    assert L.bigsi_cpu_set_rows(ix, ptr(ids), C.c_uint64(m), ptr(packed), C.c_uint64(packed.shape[1])) == 0, L.bigsi_cpu_last_error()
    return ix


def twin_rows(L, ix, m, row_bytes):
    out = np.full((m, row_bytes), 0xAB, np.uint8)
    ids = np.arange(m, dtype=np.uint64)
    assert L.bigsi_cpu_get_rows(ix, ptr(ids), C.c_uint64(m), ptr(out), C.c_uint64(row_bytes)) == 0, L.bigsi_cpu_last_error()
    return out


def twin_info(L, ix):
    inf = Info()
    assert L.bigsi_cpu_get_info(ix, C.byref(inf)) == 0
    return inf


@pytest.mark.parametrize("n", WIDTHS)
def test_twin_against_numpy(cpu, n):
    m = 257 if n < 1000 else 41
    bits = ragged_bits(m, n)
    for label, flags, keep in keep_patterns(n):
        ix = twin_index(cpu, bits)
        stride = int(twin_info(cpu, ix).row_stride_bytes)
        kept = C.c_uint64(99)
        assert cpu.bigsi_cpu_compact_columns(ix, ptr(keep), C.byref(kept)) == 0, cpu.bigsi_cpu_last_error()
        assert kept.value == int(flags.sum()) == twin_info(cpu, ix).num_cols, label
        for rb in ((n + 7) // 8, stride):          # the freed tail and the stride padding are zero
            assert np.array_equal(twin_rows(cpu, ix, m, rb), expected_rows(bits, flags, rb)), (n, label, rb)
        # out of place: the same bytes, the source untouched
        src, dst = twin_index(cpu, bits), twin_open(cpu, m, 0, 1)
        assert cpu.bigsi_cpu_extract_columns(dst, src, ptr(keep)) == 0, cpu.bigsi_cpu_last_error()
        assert twin_info(cpu, dst).num_cols == kept.value
        dstride = int(twin_info(cpu, dst).row_stride_bytes)
        assert np.array_equal(twin_rows(cpu, dst, m, dstride), expected_rows(bits, flags, dstride)), (n, label)
        assert np.array_equal(twin_rows(cpu, src, m, (n + 7) // 8), np.packbits(bits, axis=1))
        for h in (ix, src, dst):
            assert cpu.bigsi_cpu_close(h) == 0


def test_twin_error_codes(cpu):
    bits = ragged_bits(64, 100)
    keep = pack_keep(np.ones(100, bool))
    ix, other, full = twin_index(cpu, bits), twin_open(cpu, 65, 0, 1), twin_index(cpu, bits)
    empty = twin_open(cpu, 64, 0, 1)
    for rc, want in ((cpu.bigsi_cpu_compact_columns(None, ptr(keep), None), ERR_INVALID),
                     (cpu.bigsi_cpu_compact_columns(ix, None, None), ERR_INVALID),
                     (cpu.bigsi_cpu_extract_columns(None, ix, ptr(keep)), ERR_INVALID),
                     (cpu.bigsi_cpu_extract_columns(empty, None, ptr(keep)), ERR_INVALID),
                     (cpu.bigsi_cpu_extract_columns(empty, ix, None), ERR_INVALID),
                     (cpu.bigsi_cpu_extract_columns(ix, ix, ptr(keep)), ERR_INVALID),             # dst == src
                     (cpu.bigsi_cpu_extract_columns(other, ix, ptr(keep)), ERR_INVALID),          # differing m
                     (cpu.bigsi_cpu_extract_columns(full, ix, ptr(keep)), ERR_STATE)):            # non-empty dst
        assert rc == want and cpu.bigsi_cpu_last_error()
    assert cpu.bigsi_cpu_compact_columns(ix, ptr(keep), None) == 0                                # new_num_cols may be NULL
    assert np.array_equal(twin_rows(cpu, ix, 64, 13), np.packbits(bits, axis=1))
    assert np.array_equal(twin_rows(cpu, full, 64, 13), np.packbits(bits, axis=1))                # a refused call changed nothing
    for h in (ix, other, full, empty):
        assert cpu.bigsi_cpu_close(h) == 0


# --------------------------------------------------------------------------------------------- the plan's tables
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("compact_host") / "libcompact_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "compact_host.cpp")])
    lib = C.CDLL(so)
    lib.compact_host_pext.restype = C.c_uint64
    lib.compact_host_count.restype = C.c_uint64
    lib.compact_host_pext.argtypes = [C.c_uint64, C.c_void_p]
    return lib


def plan(lib, n, keep, m=1000):
    sw = (n + 63) // 64
    head, words, first = np.zeros(6, np.uint64), np.zeros((max(sw, 1), 9), np.uint64), np.zeros(sw + 2, np.uint64)
    rc = lib.compact_host_plan(C.c_uint64(n), ptr(keep), C.c_uint64(m), ptr(head), ptr(words), C.c_uint64(sw), ptr(first), C.c_uint64(sw + 2))
    assert rc == 0
    src_words, kept, dst_words, block, grid, rows = (int(x) for x in head)
    assert src_words == sw and dst_words == (kept + 63) // 64
    return dict(kept=kept, dst_words=dst_words, block=block, grid=grid, rows=rows, words=words[:sw], first=[int(x) for x in first[:dst_words + 1]])


def naive_pext(x, mask):
    out, j = 0, 0
    for b in range(64):
        if (mask >> b) & 1:
            out |= ((x >> b) & 1) << j
            j += 1
    return out


@pytest.mark.parametrize("n", WIDTHS)
def test_plan_tables_against_restatement(plan_lib, n):
    rng = np.random.default_rng(n)
    for label, flags, keep in keep_patterns(n):
        p = plan(plan_lib, n, keep)
        assert p["kept"] == int(flags.sum()) == plan_lib.compact_host_count(C.c_uint64(n), ptr(keep)), label
        sw = (n + 63) // 64
        padded = np.zeros(sw * 64, bool)
        padded[:n] = flags                                               # (junk past column n - 1 is ignored)
        before = 0
        for s in range(sw):
            mask = sum(1 << b for b in range(64) if padded[64 * s + b])
            rec = p["words"][s]
            assert (int(rec[0]), int(rec[7]), int(rec[8])) == (mask, before, bin(mask).count("1")), (label, s)
            for x in (0xFFFFFFFFFFFFFFFF, int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), 0x8000000000000001):
                assert plan_lib.compact_host_pext(C.c_uint64(x), rec.ctypes.data) == naive_pext(x, mask), (label, s, hex(x))
            before += int(rec[8])
        # first source word of a destination word: the word that holds the kept column of rank 64 o; then the last source word that keeps one
        ranks = np.flatnonzero(padded)
        assert p["first"] == [int(ranks[64 * o]) // 64 for o in range(p["dst_words"])] + [int(ranks[-1]) // 64 if ranks.size else 0], label
        assert all(p["first"][o] >= o for o in range(p["dst_words"]))          # what makes the kernel correct in place


def test_pext_network_on_corner_masks(plan_lib):
    rng = np.random.default_rng(7)
    masks = [0, 1, 1 << 63, (1 << 64) - 1, (1 << 64) - 2, (1 << 63) - 1, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0xFFFFFFFF00000000,
             0x00000000FFFFFFFF, 0x8000000000000001, 0xFF00FF00FF00FF00, 0x0123456789ABCDEF]
    masks += [int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) for _ in range(200)]
    for mask in masks:
        flags = np.array([(mask >> b) & 1 for b in range(64)], bool)
        rec = plan(plan_lib, 64, pack_keep(flags))["words"][0]
        assert int(rec[0]) == mask
        for x in [(1 << 64) - 1, mask, ~mask & ((1 << 64) - 1)] + [int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in range(4)]:
            assert plan_lib.compact_host_pext(C.c_uint64(x), rec.ctypes.data) == naive_pext(x, mask), (hex(mask), hex(x))


def replay_kernel(lib, p, src):
    """k_compact_columns' walk over one row, in Python integers: chunks of 64 destination words, a "lane" per word, which loops over
    the source words first_src[o] .. first_src[o + 1], compresses each and shifts it to (kept columns before it) - 64 o."""
    M64 = (1 << 64) - 1
    first, words, dw = p["first"], p["words"], p["dst_words"]
    out = [None] * dw
    for o in range(dw):
        acc = 0
        for s in range(first[o], first[o + 1] + 1):
            rec = words[s]
            d = int(rec[7]) - 64 * o
            if int(rec[0]) == 0 or d >= 64 or d <= -64:
                continue
            c = lib.compact_host_pext(C.c_uint64(src[s]), rec.ctypes.data)
            acc |= (c << d) & M64 if d >= 0 else c >> -d
        out[o] = acc
    return out


@pytest.mark.parametrize("n", (1, 64, 65, 129, 1025, 4097, 8193))
def test_kernel_arithmetic_replayed_from_the_tables(plan_lib, n):
    """What k_compact_columns does with the tables equals plain selection."""
    rng = np.random.default_rng(n + 5)
    row = rng.random(n) < 0.5
    padded_row = np.zeros((n + 63) // 64 * 64, bool)
    padded_row[:n] = row
    src = [sum(1 << b for b in range(64) if padded_row[64 * s + b]) for s in range((n + 63) // 64)]
    extra = [("random0.99", rng.random(n) < 0.99)]
    for label, flags, keep in keep_patterns(n) + [(l, f, pack_keep(f)) for l, f in extra]:
        p = plan(plan_lib, n, keep)
        want = row[flags[:n]]
        for o, acc in enumerate(replay_kernel(plan_lib, p, src)):
            got = np.array([(acc >> b) & 1 for b in range(64)], bool)
            chunk = want[64 * o:64 * o + 64]
            assert np.array_equal(got[:chunk.size], chunk) and not got[chunk.size:].any(), (label, o)


def test_launch_shape(plan_lib):
    keep = pack_keep(np.ones(100, bool))
    for m, block, grid in ((1, 64, 1), (8, 64, 1), (9, 128, 1), (32, 256, 1), (33, 256, 2), (4099, 256, 129), (10_000_000, 256, 1024), (1 << 40, 256, 1024)):
        p = plan(plan_lib, 100, keep, m)
        assert (p["rows"], p["block"], p["grid"]) == (8, block, grid), m
        assert p["grid"] * (p["block"] // 64) <= 4096          # about 4096 wavefronts whatever the shape


# --------------------------------------------------------------------------------------------- name lists -> keep bitmaps
def test_vacuum_plan_on_hand_made_names():
    from bigsi_amd.compact import vacuum_plan
    names = ["s%d" % c for c in range(70)]
    dead = names[:]
    for c in (0, 63, 64, 69):
        dead[c] = DELETED
    keep, kept = vacuum_plan(dead)
    flags = np.ones(70, bool)
    flags[[0, 63, 64, 69]] = False
    assert keep.dtype == np.uint8 and np.array_equal(keep, np.packbits(flags))
    assert kept == [n for c, n in enumerate(names) if flags[c]]
    keep, kept = vacuum_plan(names)                                       # none deleted
    assert np.array_equal(keep, np.packbits(np.ones(70, bool))) and kept == names
    keep, kept = vacuum_plan([DELETED] * 9)                               # all deleted
    assert np.array_equal(keep, np.zeros(2, np.uint8)) and kept == []
    assert vacuum_plan([])[1] == []


def test_extract_plan_on_hand_made_names():
    from bigsi_amd.compact import extract_plan
    names = ["s%d" % c for c in range(70)]
    names[5] = DELETED
    keep, picked = extract_plan(names, ["s69", "s0", "s64", "s63"])       # colour order, whatever order was asked for
    flags = np.zeros(70, bool)
    flags[[0, 63, 64, 69]] = True
    assert np.array_equal(keep, np.packbits(flags)) and picked == ["s0", "s63", "s64", "s69"]
    for bad, err in ((["s5"], KeyError), (["nobody"], KeyError), ([DELETED], KeyError), ([], ValueError), (["s1", "s2", "s1"], ValueError)):
        with pytest.raises(err):
            extract_plan(names, bad)


def test_keep_bytes_validation():
    from bigsi_amd.compact import keep_bytes
    flags = np.array([True, False, True] * 7)
    want = np.packbits(flags)
    assert np.array_equal(keep_bytes(flags, 21), want) and np.array_equal(keep_bytes(want, 21), want) and np.array_equal(keep_bytes(want.tobytes(), 21), want)
    for bad, err in ((flags[:20], ValueError), (want[:2], ValueError), (want.astype(np.int32), ValueError), (b"\x00", ValueError), ([1, 0], TypeError)):
        with pytest.raises(err):
            keep_bytes(bad, 21)


# --------------------------------------------------------------------------------------------- decided before any device call
def test_vacuum_and_extract_check_their_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError):
            b.vacuum(shrink=bad)
    for bad, err in (([], ValueError), (["a", "b", "a"], ValueError), ("abc", TypeError)):
        with pytest.raises(err):
            b.extract({"m": 1, "h": 1, "k": 1}, bad)


def test_abi_lists_the_new_entry_points():
    from bigsi_amd import _lib
    import re
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_compact.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.COMPACT_SIGNATURES) == ["bigsi_hip_compact_columns", "bigsi_hip_extract_columns", "bigsi_hip_shrink_to_fit"]
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.COMPACT_SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "bigsi_cpu_compact.h")).read()
    for name in ("compact_columns", "extract_columns"):
        assert "#define bigsi_hip_%s bigsi_cpu_%s" % (name, name) in header


def test_cli_parsing(tmp_path):
    from bigsi_amd.__main__ import build_parser, extract_names
    p = build_parser()[0]
    a = p.parse_args(["vacuum", "--config", "c.yaml"])
    assert (a.cmd, a.config, a.no_shrink) == ("vacuum", "c.yaml", False)
    assert p.parse_args(["vacuum", "--no-shrink"]).no_shrink is True
    a = p.parse_args(["extract", "to.yaml", "-s", "A", "-s", "B", "-c", "c.yaml"])
    assert (a.cmd, a.to_config, a.samples, a.config) == ("extract", "to.yaml", ["A", "B"], "c.yaml") and extract_names(a) == ["A", "B"]
    f = tmp_path / "names.txt"
    f.write_text("A\n\n B \nC\n")
    a = p.parse_args(["extract", "to.yaml", "--samples-file", str(f)])
    assert extract_names(a) == ["A", "B", "C"]
    with pytest.raises(ValueError):
        extract_names(p.parse_args(["extract", "to.yaml", "--samples-file", str(f), "-s", "A"]))
    with pytest.raises(SystemExit):
        p.parse_args(["extract"])


def test_cli_refuses_sharded(capsys):
    from bigsi_amd.__main__ import main
    for argv in (["vacuum", "--sharded"], ["extract", "to.yaml", "-s", "A", "--sharded"]):
        with pytest.raises(SystemExit):
            main(argv)
        assert "--sharded" in capsys.readouterr().err


class _FakeStorage(object):
    synced = 0

    def sync(self):
        self.synced += 1


class _FakeIndex(object):
    def __init__(self, n, dead):
        self.num_samples, self.dead, self.storage, self.shrink = n, dead, _FakeStorage(), None

    def vacuum(self, shrink=True):
        removed, self.shrink = self.dead, shrink
        self.num_samples -= removed
        self.dead = 0
        return removed


def test_cli_vacuum_text():
    from bigsi_amd.__main__ import vacuum_text
    ix = _FakeIndex(70, 5)
    assert json.loads(vacuum_text(ix, shrink=False)) == {"result": "removed 5 of 70 samples", "removed": 5, "num_samples": 65}
    assert ix.shrink is False and ix.storage.synced == 1
    assert json.loads(vacuum_text(ix))["result"] == "removed 0 of 65 samples" and ix.storage.synced == 1          # nothing removed: nothing written
