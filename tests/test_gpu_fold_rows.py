"""Row folding on the device: bigsi_hip_fold_rows / bigsi_hip_fold_rows_into (k_fold_rows) and bigsi_hip_trim_rows against numpy on
the very bytes written with set_rows -- expected = bitwise_or.reduce(rows.reshape(d, m', stride)), cut to the columns the index has,
read back at the full stride so that the padding is seen to be zero -- and BIGSI.fold / BIGSI.fold_into and the `fold` command against
an index BUILT under m' from the same sequences and against the oracle's model of the reference at m'.
plan_fold_rows gives a wavefront blocks of 64 destination rows at these sizes (66 for a factor of 3: whole steps of 3 rows;
tests/test_fold_rows_host.py pins that), so m' = 63, 64, 65 (66, 67 for factor 3) sit on both sides of a row-block edge."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import ROOT, assert_results_equal
from raw_index import Raw, junk_rows, ptr, rand_seq
from test_fold_rows_host import expected_fold

pytestmark = pytest.mark.gpu
_counter = itertools.count()
ERR_INVALID, ERR_RANGE, ERR_STATE = -1, -4, -6


def fold(a, factor, handle=None):
    new = C.c_uint64(1 << 60)
    return a.L.bigsi_hip_fold_rows(handle or a.ix, C.c_uint64(factor), C.byref(new)), new.value


def filled(m, n, cap, seed):
    """An index of m rows whose whole stride holds random bytes: bits beyond column n - 1 are set too (set_rows can put them there)."""
    a = Raw(m, n, cap)
    packed = junk_rows(np.random.default_rng(seed), m, n, a.stride)
    a.write(packed)
    return a, packed


# (m', factor, columns): between them every value of m' in {1, 7, 63, 64, 65, 66, 67, 4099}, of the factor in {2, 3, 4, 5, 7, 8, 9, 16,
# 17} -- every small-factor kernel, and the generic one on both sides of a group of 8 with one, eight and nine leftover rows -- and of
# the width in {1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 20000}: both sides of a word, a 128-byte line and a 1 KiB segment.
# The largest matrix is 4099 x 17 rows of 1 KiB: 71 MB.
COMBOS = [(1, 2, 1), (7, 3, 63), (63, 4, 64), (64, 5, 65), (65, 7, 1023), (4099, 8, 1024), (64, 9, 1025), (65, 16, 8191), (4099, 17, 8192),
          (66, 3, 8193), (7, 2, 20000), (4099, 2, 65), (1, 17, 1025), (67, 3, 64), (63, 6, 8193), (4099, 5, 1)]


@pytest.mark.parametrize("i", range(len(COMBOS)))
def test_a_kernel_against_numpy_in_place_and_into(i):
    new_m, d, n = COMBOS[i]
    m = new_m * d
    # strides: minimal for one of the two indexes, enlarged by the capacity for the other, alternating; the destination of the
    # out-of-place fold starts at the smallest stride there is and grows to the minimal one for n columns
    a, pa = filled(m, n, n + (5000 if i % 2 else 0), 100 + i)
    src, ps = filled(m, n, n + (0 if i % 2 else 5000), 200 + i)
    dst = Raw(new_m, 0, 1)
    try:
        assert (a.stride != src.stride) and dst.stride == 128
        rc, got_m = fold(a, d)
        assert rc == 0 and got_m == new_m == a.info().num_rows, a.L.bigsi_hip_last_error()
        assert a.info().num_cols == n and a.info().row_stride_bytes == pa.shape[1] and a.info().index_bytes == new_m * pa.shape[1]
        assert np.array_equal(a.rows(), expected_fold(pa, d, n, pa.shape[1])), COMBOS[i]
        ids = np.array([new_m], np.uint64)
        assert a.L.bigsi_hip_get_rows(a.ix, ptr(ids), 1, ptr(np.zeros(pa.shape[1], np.uint8)), pa.shape[1]) == ERR_RANGE          # rows >= m' are gone
        assert a.L.bigsi_hip_fold_rows_into(dst.ix, src.ix) == 0, a.L.bigsi_hip_last_error()
        assert dst.info().num_cols == n and dst.info().num_rows == new_m and (i % 2 or dst.stride != src.stride)          # (even i: the strides differ)
        assert np.array_equal(dst.rows(), expected_fold(ps, d, n, dst.stride)), COMBOS[i]
        assert np.array_equal(src.rows(), ps) and src.info().num_rows == m          # the source is only read
    finally:
        for r in (a, src, dst):
            r.close()


@pytest.mark.parametrize("new_m,n", [(65, 1025), (1, 63)])
def test_b_factor_one_copies_through_the_kernel(new_m, n):
    """fold_rows_into with equal row counts: a copy of the rows (bits beyond the last column dropped); fold_rows by 1 touches nothing."""
    src, ps = filled(new_m, n, n + 5000, 7)
    dst = Raw(new_m, 0, 1)
    try:
        assert fold(src, 1) == (0, new_m) and np.array_equal(src.rows(), ps)
        assert src.L.bigsi_hip_fold_rows(src.ix, C.c_uint64(1), None) == 0          # new_num_rows may be NULL
        assert src.L.bigsi_hip_fold_rows_into(dst.ix, src.ix) == 0, src.L.bigsi_hip_last_error()
        assert np.array_equal(dst.rows(), expected_fold(ps, 1, n, dst.stride)) and dst.info().num_cols == n
    finally:
        src.close()
        dst.close()


def test_c_two_folds_equal_one_fold_by_the_product():
    a, pa = filled(67 * 6, 1000, 1000, 11)
    b = Raw(67 * 6, 1000, 1000, packed=pa)
    try:
        assert fold(a, 2) == (0, 201) and fold(a, 3) == (0, 67) and fold(b, 6) == (0, 67)
        want = expected_fold(pa, 6, 1000, pa.shape[1])
        assert np.array_equal(a.rows(), want) and np.array_equal(b.rows(), want)
    finally:
        a.close()
        b.close()


def test_d_trim_rows_gives_the_memory_back():
    """Fold, then trim: the same bytes, and hipMemGetInfo shows the rows behind m' came back -- within one allocation granule, taken
    from what a small hipMalloc is seen to cost here (and from what the two matrix sizes leave of a multiple of it)."""
    from bigsi_amd import _lib
    _lib.lib()
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line))          # the runtime the library itself uses

    def free_bytes():
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return int(free.value)

    a, pa = filled(65536, 8192, 8192, 13)          # 64 MiB at a stride of 1 KiB
    try:
        p = C.c_void_p()
        f0 = free_bytes()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(1)) == 0
        granule = f0 - free_bytes()
        assert hip.hipFree(p) == 0
        assert 0 <= granule <= 64 << 20
        assert a.L.bigsi_hip_trim_rows(a.ix) == 0          # nothing to gain yet: a no-op
        assert fold(a, 4) == (0, 16384)
        want = expected_fold(pa, 4, 8192, 1024)
        assert np.array_equal(a.rows(), want)
        before = free_bytes()
        view = C.c_void_p()
        a.lib.check(a.L.bigsi_hip_open_view(a.ix, C.byref(view)))
        assert a.L.bigsi_hip_trim_rows(a.ix) == ERR_STATE and a.L.bigsi_hip_trim_rows(view) == ERR_STATE          # refused with views open, and for a view
        a.lib.check(a.L.bigsi_hip_close(view))
        assert a.L.bigsi_hip_trim_rows(a.ix) == 0, a.L.bigsi_hip_last_error()
        gained = free_bytes() - before
        assert abs(gained - (48 << 20)) <= granule, (gained, granule)
        assert np.array_equal(a.rows(), want) and a.info().num_rows == 16384
        assert a.L.bigsi_hip_trim_rows(a.ix) == 0 and free_bytes() - before == gained          # a second call is a no-op
        # the trimmed index is a whole index: it grows and folds again
        a.lib.check(a.L.bigsi_hip_reserve_cols(a.ix, 9000))
        assert fold(a, 2) == (0, 8192)
        assert np.array_equal(a.rows()[:, :1024], expected_fold(pa, 8, 8192, 1024))
    finally:
        a.close()


def test_e_refusals():
    a, pa = filled(60, 100, 100, 17)
    empty7, empty30, full, other_h = Raw(7, 0, 1), Raw(30, 0, 1), Raw(30, 5, 5), Raw(30, 0, 1, h=2)
    L = a.L
    view = C.c_void_p()
    a.lib.check(L.bigsi_hip_open_view(a.ix, C.byref(view)))
    try:
        for call, want, words in ((lambda: L.bigsi_hip_fold_rows(None, C.c_uint64(2), None), ERR_INVALID, ()),
                                  (lambda: L.bigsi_hip_fold_rows(a.ix, C.c_uint64(0), None), ERR_INVALID, ("0", "60")),
                                  (lambda: L.bigsi_hip_fold_rows(a.ix, C.c_uint64(7), None), ERR_INVALID, ("7", "60")),
                                  (lambda: L.bigsi_hip_fold_rows(view, C.c_uint64(2), None), ERR_STATE, ()),              # a view is read-only
                                  (lambda: L.bigsi_hip_fold_rows(a.ix, C.c_uint64(2), None), ERR_STATE, ("view",)),       # the owner while a view is open
                                  (lambda: L.bigsi_hip_trim_rows(view), ERR_STATE, ()),
                                  (lambda: L.bigsi_hip_trim_rows(None), ERR_INVALID, ()),
                                  (lambda: L.bigsi_hip_fold_rows_into(None, a.ix), ERR_INVALID, ()),
                                  (lambda: L.bigsi_hip_fold_rows_into(empty30.ix, None), ERR_INVALID, ()),
                                  (lambda: L.bigsi_hip_fold_rows_into(a.ix, a.ix), ERR_INVALID, ()),                      # dst == src
                                  (lambda: L.bigsi_hip_fold_rows_into(view, a.ix), ERR_STATE, ()),                        # dst a view of src
                                  (lambda: L.bigsi_hip_fold_rows_into(empty7.ix, a.ix), ERR_INVALID, ("7", "60")),        # 60 / 7 is no integer
                                  (lambda: L.bigsi_hip_fold_rows_into(a.ix, empty30.ix), ERR_INVALID, ("60", "30")),      # the ratio is below 1
                                  (lambda: L.bigsi_hip_fold_rows_into(other_h.ix, a.ix), ERR_INVALID, ("2", "3")),        # num_hashes differ
                                  (lambda: L.bigsi_hip_fold_rows_into(full.ix, a.ix), ERR_STATE, ("5",))):                # non-empty dst
            rc = call()
            msg = L.bigsi_hip_last_error().decode()
            assert rc == want and msg and all(w in msg for w in words), (rc, want, msg)
        assert np.array_equal(a.rows(), pa) and a.info().num_rows == 60 == a.info(view).num_rows          # a refused call changed nothing
        # an empty destination with a view of its own open is refused: the view's column count would go stale
        dst_view = C.c_void_p()
        a.lib.check(L.bigsi_hip_open_view(empty30.ix, C.byref(dst_view)))
        try:
            assert L.bigsi_hip_fold_rows_into(empty30.ix, a.ix) == ERR_STATE and b"view" in L.bigsi_hip_last_error()
            assert empty30.info().num_cols == 0 and not empty30.rows().any()
        finally:
            a.lib.check(L.bigsi_hip_close(dst_view))
        # a view AS THE SOURCE works
        assert L.bigsi_hip_fold_rows_into(empty30.ix, view) == 0, L.bigsi_hip_last_error()
        assert np.array_equal(empty30.rows(), expected_fold(pa, 2, 100, empty30.stride)) and empty30.info().num_cols == 100
    finally:
        a.lib.check(L.bigsi_hip_close(view))
    try:
        assert fold(a, 2) == (0, 30)                                                                       # the view is closed: now it goes
        assert np.array_equal(a.rows(), empty30.rows())
    finally:
        for r in (a, empty7, empty30, full, other_h):
            r.close()


def test_f_ipc_handles_are_refused():
    """An index attached over hipIpc in a child process is read-only: fold_rows and trim_rows get BIGSI_ERR_STATE there."""
    a, _ = filled(60, 100, 100, 19)
    try:
        handle = np.zeros(64, np.uint8)
        a.lib.check(a.L.bigsi_hip_export_ipc(a.ix, ptr(handle)))
        code = ("import ctypes as C, sys, numpy as np\n"
                "sys.path.insert(0, %r)\n"
                "from bigsi_amd import _lib\n"
                "L = _lib.lib(); h = np.frombuffer(bytes.fromhex(%r), np.uint8).copy(); ix = C.c_void_p()\n"
                "_lib.check(L.bigsi_hip_open_ipc(h.ctypes.data_as(C.c_void_p), 60, 100, 1024, 3, 0, C.byref(ix)))\n"
                "print(L.bigsi_hip_fold_rows(ix, C.c_uint64(2), None), L.bigsi_hip_trim_rows(ix))\n"
                "_lib.check(L.bigsi_hip_close(ix))\n") % (ROOT, handle.tobytes().hex())
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == [str(ERR_STATE), str(ERR_STATE)]
        assert a.info().num_rows == 60
    finally:
        a.close()


# --------------------------------------------------------------------------------------------- BIGSI level
K, M, H, N_SAMPLES = 11, 2 * 17 * 1201, 3, 40


def config(d, tag, m=M):
    return {"storage-engine": "hip-hbm", "k": K, "m": m, "h": H, "storage-config": {"name": "%s%d" % (tag, next(_counter)), "filename": str(d / ("%s%d.hbm" % (tag, next(_counter))))}}


def state_of(b):
    """(every host-side record, every row at the full stride) of an index."""
    st = b.storage
    m = int(st.res.info().num_rows)
    rows = st.res.get_rows(np.arange(m, dtype=np.uint64), int(st.res.info().row_stride_bytes))
    return {k: st[k] for k in st.record_keys()}, np.asarray(rows)


def answers(b, world):
    q = world["queries"]
    return [b.search(q[0]), b.search(q[1], 0.4), b.search(q[0], score=True), b.search(q[1], 0.4, score=True), b.search(q[1], 0.4, limit=3),
            {km: v.to01() for km, v in b.lookup(world["kmers"]).items()}, b.sample_stats(), b.similar_samples("s7"), b.similar_samples("s7", limit=4)]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """40 samples, each a mutated copy of one base sequence so that a query has many partial hits; built under M through the device
    build (real Bloom filters), and what the same sequences give under M / 2 and M / 17: a rebuilt index and the oracle's model."""
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(78)
    base = rand_seq(rng, 240)
    seqs = {}
    for c in range(N_SAMPLES):
        cut = int(rng.integers(60, 200))
        seqs["s%d" % c] = base[:cut] + rand_seq(rng, 240 - cut)
    d = tmp_path_factory.mktemp("fold")
    queries = [base[:100], base[:200]]
    made = []
    w = {"dir": d, "seqs": seqs, "queries": queries, "kmers": list(dict.fromkeys(seq_to_kmers(base[:40], K))), "made": made, "rebuilt": {}, "model": {}}
    yield w
    for x in made:
        x.delete()


def build(world, tag, m=M):
    from bigsi_amd import BIGSI
    b = BIGSI.build_from_sequences(config(world["dir"], tag, m), {n: [s] for n, s in world["seqs"].items()})
    world["made"].append(b)
    return b


def rebuilt(world, new_m):
    if new_m not in world["rebuilt"]:
        world["rebuilt"][new_m] = build(world, "rebuilt", new_m)
    return world["rebuilt"][new_m]


def model(world, new_m):
    from bigsi_amd.utils import seq_to_kmers
    from oracle.ref_model import OracleBIGSI
    if new_m not in world["model"]:
        names = list(world["seqs"])
        world["model"][new_m] = OracleBIGSI.build([OracleBIGSI.bloom(seq_to_kmers(world["seqs"][n], K), new_m, H) for n in names], names, K, new_m, H)
    return world["model"][new_m]


def check_against_rebuild_and_model(b, world, new_m, deleted=()):
    fresh, orc = rebuilt(world, new_m), model(world, new_m)
    (kv1, rows1), (kv2, rows2) = state_of(b), state_of(fresh)
    assert rows1.shape == rows2.shape and np.array_equal(rows1, rows2)
    assert np.array_equal(rows1[:, :orc.rb], orc.rows) and not rows1[:, orc.rb:].any()
    assert int(b.bloomfilter_size) == new_m == int(b.storage.res.info().num_rows) == b.bitmatrix.num_rows == int(b.storage.get_integer("number_of_rows"))
    got = answers(b, world)
    if not deleted:
        assert kv1 == kv2
        assert got == answers(fresh, world)
    q = world["queries"]
    names = [n if n not in deleted else "D3L3T3D" for n in world["seqs"]]
    orc.names = names
    try:
        for r, (s, thr, score) in zip(got[:4], ((q[0], 1.0, False), (q[1], 0.4, False), (q[0], 1.0, True), (q[1], 0.4, True))):
            assert_results_equal(r, orc.search(s, thr, score), "m'=%d t=%r score=%r" % (new_m, thr, score))
            assert len(r) > 3
        assert_results_equal(got[4], orc.search(q[1], 0.4)[:3], "limit")
        assert got[5] == orc.lookup(world["kmers"])
        bits = np.unpackbits(orc.rows, axis=1)[:, :N_SAMPLES].sum(axis=0)
        assert [(r["sample_name"], r["bits_set"]) for r in got[6]] == [(n, int(bits[c])) for c, n in enumerate(names) if n != "D3L3T3D"]
        assert all(r["fill"] == r["bits_set"] / new_m for r in got[6])
        # similar_samples("s7") restated in numpy on the model's rows: A = bits of s7's filter, X = bits of each sample's, I = shared
        colbits = np.unpackbits(orc.rows, axis=1)[:, :N_SAMPLES].astype(bool)
        a, x, i = int(bits[7]), [int(v) for v in bits], [int(v) for v in (colbits & colbits[:, 7:8]).sum(axis=0)]
        want = [{"sample_name": n, "colour": c, "bits_shared": i[c], "jaccard": i[c] / (a + x[c] - i[c]) if a + x[c] - i[c] else 0.0,
                 "containment": i[c] / a if a else 0.0} for c, n in enumerate(names) if n != "D3L3T3D" and c != 7]
        want.sort(key=lambda r: -r["jaccard"])          # stable: ties stay in ascending colour
        assert got[7] == want and got[8] == want[:4] and len(want) == N_SAMPLES - 1 - len(deleted)
    finally:
        orc.names = list(world["seqs"])
    for r in (new_m, new_m + 5):                                                                           # rows >= m' are gone, as any row out of range
        with pytest.raises(KeyError):
            b.storage.res.get_rows([r])


@pytest.mark.parametrize("factor", [2, 17])
def test_g_fold_in_place_equals_the_index_built_under_the_smaller_size(world, factor):
    b = build(world, "main")
    old_bytes = M * int(b.storage.res.info().row_stride_bytes)
    out = b.fold(factor, trim=(factor == 2))
    assert out == {"m": M // factor, "factor": factor, "trimmed": factor == 2}
    assert int(b.storage.res.info().index_bytes) == old_bytes // factor
    check_against_rebuild_and_model(b, world, M // factor)
    assert b.fold(1) == {"m": M // factor, "factor": 1, "trimmed": False}                                 # nothing to do, nothing touched


def test_h_fold_into_keeps_deleted_samples_deleted(world):
    from bigsi_amd import BIGSI
    b = build(world, "src")
    b.delete_sample("s3")
    b.delete_sample("s39")
    d = world["dir"]
    new = b.fold_into(config(d, "into", M // 34), 34)
    world["made"].append(new)
    assert new.num_samples == N_SAMPLES and new.sample_to_colour("s4") == 4 and new.colour_to_sample(3) == "D3L3T3D"
    with pytest.raises(KeyError):
        new.similar_samples("s3")
    check_against_rebuild_and_model(new, world, M // 34, deleted=("s3", "s39"))
    assert int(b.bloomfilter_size) == M == int(b.storage.res.info().num_rows) and b.num_samples == N_SAMPLES          # the source is as it was
    kv_new, kv_src = state_of(new)[0], state_of(b)[0]
    assert {k: v for k, v in kv_new.items() if k.startswith("metadata:")} == {k: v for k, v in kv_src.items() if k.startswith("metadata:")}
    for bad_cfg, factor in ((config(d, "never", M // 2), 17), (dict(config(d, "never", M // 2), h=2), 2), (dict(config(d, "never", M // 2), k=9), 2)):
        with pytest.raises(ValueError):
            b.fold_into(bad_cfg, factor)
    from bigsi_amd._lib import BigsiHipError
    with pytest.raises((ValueError, BigsiHipError)):
        b.fold_into(dict(b.config, m=M // 2), 2)                                                           # a storage name of its own (the storage layer says so first)
    with pytest.raises(ValueError):
        b.fold_into(new.config, 34)                                                                        # not empty
    assert BIGSI(new.config).num_samples == N_SAMPLES                                                     # (refusing it did not empty it)


def test_i_live_batch_sees_the_folded_index(world):
    """A batch created and run before fold_rows, then reloaded and run after it, returns the folded index's hits: a run takes the
    index's geometry at that moment."""
    b = build(world, "live")
    st = b.storage
    batch = st.new_batch(world["queries"], K)
    batch.run(0.4)
    off0, col0, cnt0 = (np.array(x) for x in batch.hits())
    assert st.fold_rows(17) == M // 17
    batch.reload(world["queries"], K)
    batch.run(0.4)
    off1, col1, cnt1 = (np.array(x) for x in batch.hits())
    fresh = rebuilt(world, M // 17)
    fb = fresh.storage.new_batch(world["queries"], K)
    fb.run(0.4)
    off2, col2, cnt2 = (np.array(x) for x in fb.hits())
    assert np.array_equal(off1, off2) and np.array_equal(col1, col2) and np.array_equal(cnt1, cnt2)
    assert int(off0[-1]) <= int(off1[-1]) and not (np.array_equal(off0, off1) and np.array_equal(cnt0, cnt1))          # (17 x fewer rows: more k-mers found)
    batch.close()
    fb.close()


def test_j_groups_are_refused(tmp_path):
    from bigsi_amd import BIGSI
    from bigsi_amd._lib import BigsiHipError
    rng = np.random.default_rng(10)
    cfg = {"storage-engine": "hip-hbm", "k": K, "m": 1000, "h": H, "storage-config": {"name": "foldgrp%d" % next(_counter), "devices": [0, 0], "max_cols": 8}}
    b = BIGSI.build_from_sequences(cfg, {"g%d" % c: [rand_seq(rng, 60)] for c in range(6)})
    try:
        for call in (lambda: b.fold(2), lambda: b.fold_into(config(tmp_path, "never", 500), 2), lambda: b.storage.fold_rows(2), b.storage.trim_rows):
            with pytest.raises(BigsiHipError) as e:
                call()
            assert e.value.code == ERR_STATE
        assert int(b.bloomfilter_size) == 1000 and int(b.storage.res.info().num_rows) == 1000
    finally:
        b.delete()


def test_k_snapshot_of_a_folded_index(world, tmp_path):
    """fold -> sync() -> drop -> reopen under the new config: m' rows, identical bytes and results, an allocation of m' rows; the
    config from before the fold is refused, for the resident index and for its snapshot."""
    from bigsi_amd import BIGSI
    from bigsi_amd._lib import BigsiHipError
    from bigsi_amd.storage.hip_hbm import HipHbmStorage
    b = build(world, "snap")
    old_cfg = b.config
    assert b.fold(2, trim=False)["trimmed"] is False
    new_cfg = dict(old_cfg, m=M // 2)
    b.storage.sync()
    want_state, want_answers = state_of(b), answers(b, world)
    with pytest.raises(BigsiHipError) as e:
        BIGSI(old_cfg)                                                                                     # resident: the name is an index of m' rows now
    assert "m=" in str(e.value)
    name = old_cfg["storage-config"]["name"]
    HipHbmStorage.drop(name)
    with pytest.raises(BigsiHipError) as e:
        BIGSI(old_cfg)                                                                                     # from the snapshot
    assert "number_of_rows %d differs from the index in the snapshot %s (%d rows)" % (M, old_cfg["storage-config"]["filename"], M // 2) in str(e.value)
    again = BIGSI(new_cfg)
    world["made"][world["made"].index(b)] = again
    got_state = state_of(again)
    assert got_state[0] == want_state[0] and np.array_equal(got_state[1], want_state[1])
    assert answers(again, world) == want_answers
    inf = again.storage.res.info()
    assert int(inf.num_rows) == M // 2 and int(inf.index_bytes) == (M // 2) * int(inf.row_stride_bytes)
    check_against_rebuild_and_model(again, world, M // 2)


def test_l_cli_fold(world, tmp_path, capsys):
    """`python -m bigsi_amd fold` in processes of their own on an index's snapshot: --dry-run, out of place and --in-place, each followed
    by a `search` under the new config that prints what `search` prints for the index built under m'."""
    from bigsi_amd.__main__ import main
    from bigsi_amd.storage.hip_hbm import HipHbmStorage
    b = build(world, "cli")
    cfg = b.config
    fresh = rebuilt(world, M // 2)
    to, inplace = config(tmp_path, "clito", M // 2), dict(cfg, m=M // 2)
    HipHbmStorage.drop(cfg["storage-config"]["name"])                     # (the snapshot is what the child processes see)
    files = {}
    for tag, c in (("c", cfg), ("to", to), ("inplace", inplace), ("fresh", fresh.config)):
        files[tag] = tmp_path / ("%s.yaml" % tag)
        files[tag].write_text(yaml.safe_dump(c))

    def child(*argv):
        r = subprocess.run([sys.executable, "-m", "bigsi_amd"] + list(argv), cwd=str(tmp_path), capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    def here(*argv):
        capsys.readouterr()
        assert main(list(argv)) == 0
        return capsys.readouterr().out

    q = world["queries"][1]
    want = here("search", q, "-t", "0.4", "--config", str(files["fresh"]))
    assert len(json.loads(want)["results"]) > 3
    try:
        dry = json.loads(child("fold", "--factor", "2", "--dry-run", "--config", str(files["c"])))
        assert list(dry) == ["m", "factor", "valid", "new_m", "factors_near", "note", "estimate"]
        assert (dry["m"], dry["valid"], dry["new_m"]) == (M, True, M // 2) and [2, M // 2] in dry["factors_near"] and len(dry["estimate"]) == N_SAMPLES
        exact = {r["sample_name"]: r for r in fresh.sample_stats()}
        for r in dry["estimate"]:                                         # the estimate is a model; the folded index's stats are the truth: within 6 sigma
            p, x = r["est_fill"], exact[r["sample_name"]]["bits_set"]
            assert abs(x - (M // 2) * p) <= 6 * ((M // 2) * p * (1 - p)) ** 0.5
        out = json.loads(child("fold", str(files["to"]), "--factor", "2", "--config", str(files["c"])))
        assert (out["m"], out["factor"], out["num_samples"]) == (M // 2, 2, N_SAMPLES) and str(files["to"]) in out["result"]
        assert here("search", q, "-t", "0.4", "--config", str(files["to"])) == want
        out = json.loads(child("fold", str(files["inplace"]), "--factor", "2", "--in-place", "--config", str(files["c"])))
        assert (out["m"], out["factor"], out["trimmed"]) == (M // 2, 2, True)
        assert here("search", q, "-t", "0.4", "--config", str(files["inplace"])) == want
    finally:
        world["made"].remove(b)
        from bigsi_amd import BIGSI
        for c in (to, inplace):
            if os.path.exists(c["storage-config"]["filename"]):
                BIGSI(c).delete()
