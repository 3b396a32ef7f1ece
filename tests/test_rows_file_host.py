"""The file side of bulk ingest and snapshots without a GPU (bigsi_amd/csrc/bigsi_rowsfile.cpp: plain host C++): the flat file, the
striped directory and the threaded BerkeleyDB row gather with its scan cache, driven by tests/c_host/rowsfile_host.cpp -- a program
with its own main, built by g++ once with AddressSanitizer + UndefinedBehaviorSanitizer and once with ThreadSanitizer (the code is
threaded, the scan cache a mutex-guarded global) and run as a process of its own.  Nothing sanitized is loaded into Python.  What the
program gathers from a store libdb wrote is compared here with the Python page walk (bigsi_amd/bdb.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
              "tsan": ["-fsanitize=thread", "-static-libtsan"]}          # (the runtimes are part of the program: no library order to get wrong)
ROW0, N, ROW_BYTES = 5, 690, 4500


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rowsfile_" + request.param) / "rowsfile_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZERS[request.param] +
                          ["-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "c_host", "rowsfile_host.cpp"),
                           os.path.join(ROOT, "bigsi_amd", "csrc", "bigsi_rowsfile.cpp"), "-lpthread"])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-4000:])
    return r.stdout


def test_flat_file_and_striped_directory_against_the_naive_model(exe, tmp_path):
    assert run(exe, "files", tmp_path).strip() == "rows file host: ok"
    assert os.listdir(tmp_path) == []          # (it removes its files: some 350 MB)


# --------------------------------------------------------------------------------------------- rows of a BerkeleyDB store
def store_records(seed):
    """700 row records of lengths 3, 4071, 4096 and 5000 (inline, and overflow chains around the 4 KiB page) less a gap of missing
    rows, and a few records that are no rows."""
    rng = np.random.default_rng(seed)
    rec = {b"number_of_rows:int": b"700", b"number_of_cols:int": b"40000", b"empty:string": b"", b"metadata:7:string": "séven".encode(),
           b"blob:string": rng.integers(0, 256, size=30000, dtype=np.uint8).tobytes(), b"12:bitarrayX": b"not a row", b"x12:bitarray": b"nor this"}
    for i in range(700):
        if not 300 + seed <= i < 320 + 2 * seed:
            rec[b"%d:bitarray" % i] = rng.integers(0, 256, size=int(rng.choice([3, 5000, 4071, 4096])), dtype=np.uint8).tobytes()
    return rec


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    ndbm = pytest.importorskip("dbm.ndbm")
    if getattr(ndbm, "library", "") != "Berkeley DB":          # (the rule of tests/test_bdb_reader.py)
        pytest.skip("dbm.ndbm is not backed by Berkeley DB here")
    from bigsi_amd.bdb import read_all
    d = tmp_path_factory.mktemp("rowsfile_stores")
    out = []
    for seed in (1, 2):
        db = ndbm.open(str(d / ("s%d" % seed)), "n")
        for k, v in store_records(seed).items():
            db[k] = v
        db.close()
        fn = str(d / ("s%d.db" % seed))
        out.append((fn, read_all(fn)))
    return out


def expected_rows(records):
    """Rows [ROW0, +N) as the Python page walk reads them: cut or zero-extended to ROW_BYTES, zeros for a row the store does not hold."""
    want = np.zeros((N, ROW_BYTES), np.uint8)
    for i in range(N):
        v = records.get(b"%d:bitarray" % (ROW0 + i), b"")[:ROW_BYTES]
        want[i, :len(v)] = np.frombuffer(v, np.uint8)
    return want


def small_of(records):
    return {k: v for k, v in records.items() if not (k.endswith(b":bitarray") and k[:-9].isdigit())}


def parse_small(path):
    raw, out, at = open(path, "rb").read(), {}, 0
    while at < len(raw):
        kl, vl = struct.unpack_from("<II", raw, at)
        out[raw[at + 8:at + 8 + kl]] = raw[at + 8 + kl:at + 8 + kl + vl]
        at += 8 + kl + vl
    return out


@pytest.mark.parametrize("threads", [1, 4])
def test_berkeleydb_rows_plain_cached_and_after_a_rewrite(exe, stores, tmp_path, threads):
    import shutil
    (fn1, rec1), (fn2, rec2) = stores
    assert len(rec1) != len(rec2) and not np.array_equal(expected_rows(rec1), expected_rows(rec2))
    assert expected_rows(rec1)[300 + 1 - ROW0:320 + 2 - ROW0].any() == 0 and expected_rows(rec1).any(axis=1).sum() == N - 21
    store = str(tmp_path / "store.db")          # (the rewritten route overwrites it)
    shutil.copy(fn1, store)
    got = {}
    for route, other in (("plain", None), ("cached", None), ("rewritten", fn2)):
        out = str(tmp_path / route)
        text = run(exe, "bdb", store, ROW0, N, ROW_BYTES, threads, route, out, *([other] if other else []))
        got[route] = np.fromfile(out + ".rows", np.uint8).reshape(N, ROW_BYTES)
        if route != "plain":          # the scan saw the first store
            assert parse_small(out + ".small") == small_of(rec1)
            assert text.split() == ["rows", str(sum(1 for k in rec1 if k not in small_of(rec1))), "widest", "5000"]
    assert np.array_equal(got["plain"], expected_rows(rec1))
    assert np.array_equal(got["cached"], got["plain"])
    assert np.array_equal(got["rewritten"], expected_rows(rec2))          # the scan of the first store was not used
