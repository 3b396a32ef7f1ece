"""CPU-only: the launch rule of the hit-list compaction and the size of the pinned export (plan_hits, export_spec in
bigsi_amd/csrc/bigsi_launch.hpp) compiled as plain host C++ (tests/c_host/hits_plan_host.cpp): the constants and the shapes the header
states, pinned, and the invariants over a seeded sweep.  A GPU test compares results, which a slip in the rule leaves right -- until a
hit sits on a cut the slip moved.  The rule and the walk of its workgroups and threads also run in a stand-alone program under
AddressSanitizer and UBSan (tests/c_host/hits_sanitize_main.cpp)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def build_hits_host(tmp_path):
    so = str(tmp_path / "libhits_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "hits_plan_host.cpp")])
    L = C.CDLL(so)
    L.hits_host_export_spec.restype = C.c_uint64
    return L


def plan(L, nchunks, n_shards=1):
    """(items per group, groups, single-workgroup body)"""
    out = np.zeros(3, np.uint64)
    L.hits_host_plan(C.c_uint64(nchunks), C.c_uint32(n_shards), out.ctypes.data_as(C.c_void_p))
    return int(out[0]), int(out[1]), bool(out[2])


def spec(L, n_seqs, capacity):
    return int(L.hits_host_export_spec(C.c_uint64(n_seqs), C.c_uint64(capacity)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_hits_host(tmp_path_factory.mktemp("hits_host"))


def test_shipped_constants(lib):
    """At most 1024 workgroups; up to 16 items go to one; lists of 65 536 entries to start with; the export carries 16 hits per
    sequence, at least 1024 and at most 2^20; an item is the 256 words of a workgroup's threads."""
    out = np.zeros(7, np.uint64)
    lib.hits_host_constants(out.ctypes.data_as(C.c_void_p))
    assert out.tolist() == [1024, 16, 65536, 1024, 16, 1 << 20, 256]


def test_pinned_shapes(lib):
    # 16 items: one workgroup that owns them all, the single-workgroup body; 17: one item per workgroup
    assert plan(lib, 16) == (16, 1, True) and plan(lib, 17) == (1, 17, False)
    assert [plan(lib, n) for n in (1, 2, 7)] == [(1, 1, True), (2, 1, True), (7, 1, True)]
    # 1024 items fill the grid one each; 1025 take two each and leave the last workgroup one; 2100: three each, a last group of 3
    assert plan(lib, 1024) == (1, 1024, False) and plan(lib, 1025) == (2, 513, False) and plan(lib, 2100) == (3, 700, False)
    assert plan(lib, 2048) == (2, 1024, False) and plan(lib, 2049) == (3, 683, False)
    # the host's bound on the number of items
    assert plan(lib, 0x7FFFFFFF) == (2097152, 1024, False)
    # gathered shards never take the single-workgroup body, whatever the number of items; the grid does not depend on the shards
    assert plan(lib, 16, 3) == (16, 1, False) and plan(lib, 3, 3) == (3, 1, False) and plan(lib, 17, 3) == (1, 17, False)
    # no item: one workgroup that owns nothing (never launched by the library)
    assert plan(lib, 0) == (1, 1, True)
    # the export: 1024 for up to 64 sequences, 16 n beyond, capped by the lists (65 536 entries until they grow) and by 2^20
    assert [spec(lib, n, 65536) for n in (0, 1, 64, 65, 257, 300, 4096, 4097, 16400)] == [1024, 1024, 1024, 1040, 4112, 4800, 65536, 65536, 65536]
    assert spec(lib, 16400, 262400) == 262400 and spec(lib, 16400, 300000) == 262400
    assert spec(lib, 65536, 1 << 21) == 1 << 20 and spec(lib, 65537, 1 << 21) == 1 << 20 and spec(lib, 65535, 1 << 21) == (1 << 20) - 16
    assert spec(lib, 1, 1000) == 1000 and spec(lib, 1, 0) == 0 and spec(lib, 1, 65537) == 1024


def test_invariants_over_a_seeded_sweep(lib):
    """groups <= 1024 and groups x ipb >= nchunks > (groups - 1) x ipb: every workgroup owns an item and the last one ends the
    list; one workgroup exactly up to 16 items; beyond, ipb = ceil(nchunks / 1024)."""
    rng = random.Random(11)
    sizes = list(range(1, 3000)) + [rng.randrange(1, 1 << rng.randrange(1, 32)) for _ in range(6000)] + [0x7FFFFFFF, 0x7FFFFFFE, 1 << 30]
    one = many = 0
    for n in sizes:
        n = min(n, 0x7FFFFFFF)
        shards = rng.choice([1, 1, 2, 3, 8])
        ipb, groups, single = plan(lib, n, shards)
        assert 1 <= groups <= 1024 and groups * ipb >= n > (groups - 1) * ipb, n
        assert (groups == 1) == (n <= 16) and single == (groups == 1 and shards == 1), n
        assert ipb == (n if n <= 16 else -(-n // 1024)), n
        one += groups == 1
        many += ipb > 1 and groups > 1
    assert one >= 16 and many > 3000
    for _ in range(3000):
        n, cap = rng.randrange(0, 1 << rng.randrange(1, 33)), rng.choice([65536, rng.randrange(0, 1 << rng.randrange(1, 40))])
        assert spec(lib, n, cap) == min(max(1024, 16 * n), cap, 1 << 20), (n, cap)


def test_library_binds_the_hits_hook():
    """The device library exports bigsi_hip_hits_last_path with the binding's argument types (loading it needs no GPU); the binding's
    structure has the header's fields in the header's order."""
    import re
    from bigsi_amd import _lib
    fn = _lib.lib().bigsi_hip_hits_last_path
    assert fn.argtypes[:2] == [C.c_void_p, C.c_uint32] and fn.restype == C.c_int
    src = open(os.path.join(ROOT, "include", "bigsi_hip_testing.h")).read()
    body = re.search(r"typedef struct bigsi_hip_hits_path \{\s*uint32_t ([^;]+);\s*\} bigsi_hip_hits_path;", src).group(1)
    assert [f.strip() for f in body.split(",")] == [name for name, _ in _lib.HitsPath._fields_]
    assert C.sizeof(_lib.HitsPath) == 4 * len(_lib.HitsPath._fields_)
    for name, value in (("BATCH", 0), ("INDEX", 1), ("GROUP_BATCH", 2)):
        assert "#define BIGSI_HITS_PATH_OF_%s %du" % (name, value) in src and getattr(_lib, "HITS_PATH_OF_" + name) == value
    # a NULL owner and an unknown kind are refused before anything is read
    out = _lib.HitsPath()
    assert fn(None, 0, C.byref(out)) == _lib.ERR_INVALID


def test_sanitized_program_over_the_plan_and_its_walks(tmp_path):
    """tests/c_host/hits_sanitize_main.cpp -- a program with its own main that walks every plan's workgroups over an array of exactly
    as many items, and the single-workgroup body's threads over a vector of exactly as many words -- built with AddressSanitizer and
    UBSan and run as a program: it must end clean."""
    exe = str(tmp_path / "hits_sanitize")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "c_host", "hits_sanitize_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "hit-list plan, its walks and the export's size: ok" and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
