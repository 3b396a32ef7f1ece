"""k_rank_select -- the kernel behind limit=N -- bit for bit against numpy (tests/rank_cases.py; its reference and every case's edge
are pinned on the CPU by tests/test_rank_cases_host.py), in two layers.

Layer D, the kernel alone through bigsi_hip_rank_select_arrays: arrays of a few KB whose contents are chosen, many queries per
call, one workgroup each.  The early return (total = limit - 1, limit, limit + 1, 0; the exclusion alone reaching the limit); exact
runs of 1, 2, 255, 256, 257, 513 and 600 words with the cut at the first and last bit of a word, inside a byte, on the lane 63 | 64
edge of the scan, on the tile edges 255 | 256 and 511 | 512, in the ragged last word, and limit = 1 with the only hits in the last
tile; one digit (all counts at min_kmers, all at num_unique, the cutoff in bins 0, 15, 16, 1023, 1024 and 4095 with one, some and all
of the bin fitting); two digits (range 4096 and 8192 around 4095 | 4096 | 4097 and 8191 | 8192, 16-bit counters at 65 535, 32-bit ones
at 65 536 and 65 537); three digits (range 2^24 - 1: two passes; 2^24 and beyond: three, with pairs that differ in one digit only);
ties interleaved with higher counts and ties in tiles 0 and 2 with none in tile 1; excluded colours at column 0, 63, 64 and the last
one, as every hit of a word, among the higher counts, inside the tie block and beyond the vector; and three seeded calls of 512
queries each.  The counter of every column that is not a hit holds all ones; every case runs out of place -- into a buffer preset to
a pattern -- and in place, and the words behind wv must come back as they went in.

Layer E, the wiring, on staircase indexes (tests/count_staircase.py with chosen columns) that carry a tie block across columns 61 ..
66, 16 380 .. 16 390 and the last columns of the index, higher counts before, between and behind: put_rows, set_limit, run, hits(),
with colours and counts of the main query and every filler against the reference; limits that put the cut on each of those places and
at T - 1, T, T + 1 of the main query's hits; excluded colours from the block and from the higher counts.  Sliced 16-bit, one slice,
sparse counters after a threshold-0.0 run has filled them all, two digits (u = 65 530 at threshold 0.0), 32-bit, 513 words thresholded
and exact, the same index as a group of two shards of 257 words (the members trim in place, the host merge cuts the union), and one
streamed run in small chunks."""
import itertools
import time
from collections import OrderedDict

import numpy as np
import pytest

import rank_cases as rc
from count_staircase import K, min_kmers

pytestmark = pytest.mark.gpu
_counter = itertools.count()


@pytest.fixture(scope="module")
def hip():
    import bigsi_amd
    from bigsi_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible"
    t0 = time.perf_counter()
    yield bigsi_amd
    print("test_gpu_rank_select wall time: %.1f s" % (time.perf_counter() - t0))


# --------------------------------------------------------------------------------------------- layer D
def rank_select_arrays(hits, wv, counters, nu, mk, excluded_words, limit, in_place, out):
    from bigsi_amd import _lib
    n, stride = hits.shape
    _lib.check(_lib.lib().bigsi_hip_rank_select_arrays(0, _lib.ptr(hits), stride, wv, n, _lib.ptr(counters), 0 if counters is None else counters.itemsize,
                                                        _lib.ptr(nu), _lib.ptr(mk), _lib.ptr(excluded_words), limit, int(in_place), _lib.ptr(out)))
    return out


def run_call(hits, wv, counters, nu, mk, excluded, limit, names):
    """one call's arrays, out of place into a preset buffer and in place, against the reference query by query"""
    n, stride = hits.shape
    ex_words = rc.words_of(excluded, wv) if excluded else None
    nu32, mk32 = np.ascontiguousarray(nu, np.uint32), np.ascontiguousarray(mk, np.uint32)
    before = hits.copy()
    for in_place in (False, True):
        out = np.full((n, stride), rc.PRESET, np.uint64)
        rank_select_arrays(hits, wv, counters, nu32, mk32, ex_words, limit, in_place, out)
        assert np.array_equal(hits, before)          # (the caller's arrays are inputs)
        for q in range(n):
            want = rc.reference(hits[q], None if counters is None else counters[q], int(nu[q]), int(mk[q]), excluded, limit, wv=wv,
                                preset=None if in_place else np.full(stride, rc.PRESET, np.uint64))
            if not np.array_equal(out[q], want):
                w = np.flatnonzero(out[q] != want)
                raise AssertionError("%s (query %d, wv %d, limit %d, in_place %d): words %s differ: got %s, want %s"
                                     % (names[q], q, wv, limit, in_place, w[:6].tolist(), [hex(int(x)) for x in out[q][w[:6]]], [hex(int(x)) for x in want[w[:6]]]))


@pytest.mark.parametrize("group", rc.DIRECT_GROUPS)
def test_direct_cases_equal_numpy(hip, group):
    calls = OrderedDict()
    for c in rc.DIRECT:
        if c["group"] == group:
            calls.setdefault(rc.call_key(c), []).append(c)
    assert calls
    rng = np.random.default_rng(17)
    for (wv, limit, excluded, cbytes), cases in calls.items():
        stride = wv + rc.PAD
        junk = rng.integers(0, 1 << 63, size=(len(cases), rc.PAD), dtype=np.int64).astype(np.uint64)          # hit words behind wv: not the kernel's
        hits = np.ascontiguousarray(np.concatenate([np.stack([rc.words_of(c["cols"], wv) for c in cases]), junk], axis=1))
        counters = np.stack([c["counts"] for c in cases]).astype(np.uint32 if cbytes == 4 else np.uint16) if cbytes else None
        run_call(hits, wv, counters, [c["nu"] for c in cases], [c["mk"] for c in cases], excluded, limit, [c["name"] for c in cases])


@pytest.mark.parametrize("cbytes", [2, 4, 0])
def test_seeded_fuzz_equals_numpy(hip, cbytes):
    f = rc.fuzz_call(100 + cbytes, n_seqs=512, wv=600, cbytes=cbytes)
    run_call(f["hits"], f["wv"], f["counts"], f["nu"], f["mk"], f["excluded"], f["limit"], ["fuzz %d" % q for q in range(512)])


def test_refusals_come_before_any_device_work(hip):
    from bigsi_amd import _lib
    L = _lib.lib()
    hits, out = np.zeros((2, 4), np.uint64), np.full((2, 4), rc.PRESET, np.uint64)
    cnt, nu = np.zeros((2, 256), np.uint16), np.zeros(2, np.uint32)
    good = [0, _lib.ptr(hits), 4, 3, 2, _lib.ptr(cnt), 2, _lib.ptr(nu), _lib.ptr(nu), None, 5, 0, _lib.ptr(out)]
    for i, bad in ((1, None), (12, None), (3, 5), (6, 3), (6, 8), (10, 0), (7, None), (8, None)):
        args = list(good)
        args[i] = bad
        assert L.bigsi_hip_rank_select_arrays(*args) == _lib.ERR_INVALID, (i, bad)
        assert (out == rc.PRESET).all()
    assert L.bigsi_hip_rank_select_arrays(*good) == _lib.OK and not out[:, :3].any() and (out[:, 3] == rc.PRESET).all()


# --------------------------------------------------------------------------------------------- layer E
def open_index(c, sc):
    from bigsi_amd.storage import get_storage
    cfg = {"name": "rank%d" % next(_counter), "max_cols": c["n_cols"]}
    if c["devices"]:
        cfg["devices"] = c["devices"]
    st = get_storage({"storage-engine": "hip-hbm", "k": K, "m": c["m"], "h": c["h"], "storage-config": cfg})
    st.delete_all()
    for key, v in (("number_of_rows", c["m"]), ("number_of_cols", c["n_cols"]), ("ksi:bloomfilter_size", c["m"]), ("ksi:num_hashes", c["h"])):
        st.set_integer(key, v)
    st.res.put_rows(sc.row_ids, sc.packed)
    return st


_refs = {}


def references(name):
    """([u of every query], int32[n_queries, n_cols]) from Staircase.reference: once per index, shared, never changed"""
    c, sc, queries, _, _ = rc.build_stair(name)
    key = (c["base"], c["main_pos"])
    if key not in _refs:
        pairs = [sc.reference(q) for q in queries]
        _refs[key] = (np.array([u for u, _ in pairs], np.int64), np.stack([cnt for _, cnt in pairs]).astype(np.int32))
        _refs[key][1].setflags(write=False)
    return _refs[key]


def orders_of(us, ref, mks, exact, excluded):
    """per query the hits in the order a limited search cuts them"""
    out = []
    for i in range(len(us)):
        hit = np.flatnonzero(ref[i] == us[i]) if exact else np.flatnonzero(ref[i] >= mks[i])
        if exact and us[i] == 0:
            hit = hit[:0]
        out.append(rc.ranked_order(hit, ref[i][hit], excluded, exact))
    return out


def check_hits(got, us, ref, orders, limit, exact, what):
    off, col, cnt = got
    off = off.astype(np.int64)
    want = [np.sort(o[:limit]) for o in orders]
    lens = np.array([w.size for w in want])
    bad = np.flatnonzero(np.diff(off) != lens)
    assert bad.size == 0, (what, "hits per query", bad[:8], np.diff(off)[bad[:8]], lens[bad[:8]])
    flat = np.concatenate(want) if want else np.zeros(0, np.int64)
    qi = np.repeat(np.arange(len(want)), lens)
    assert np.array_equal(col, flat), (what, "colours", qi[np.flatnonzero(col != flat)[:8]], col[np.flatnonzero(col != flat)[:8]], flat[np.flatnonzero(col != flat)[:8]])
    wcnt = us[qi] if exact else ref[qi, flat]
    assert np.array_equal(cnt, wcnt), (what, "counts", qi[np.flatnonzero(cnt != wcnt)[:8]])


def excluded_sets(sc, tie, counts, mk, exact):
    """no exclusion; colours from the tie block and from the higher counts (and two beyond the index, which must change nothing)"""
    block = rc.tie_block(sc.n_cols)
    high = np.flatnonzero(counts > tie)
    ex = [block[0], block[2], block[-1], int(high[0]), int(high[-1]), sc.n_cols + 5, 10 ** 6]
    if sc.n_cols > 16390:
        ex += [16383, 16384]
    if exact:
        full = np.flatnonzero(counts == sc.u)
        ex += [int(full[0]), int(full[len(full) // 2])]
    return [(), tuple(sorted(set(ex)))]


@pytest.mark.parametrize("name", [c["name"] for c in rc.STAIR_CASES])
def test_limited_runs_on_a_staircase_equal_numpy(hip, name):
    c, sc, queries, thr, tie = rc.build_stair(name)
    us, ref = references(name)
    exact = c["exact"]
    run_thr = 1.0 if exact else thr
    mks = np.array([min_kmers(int(u), thr) for u in us], np.int64)
    st = open_index(c, sc)
    batch = st.new_batch(queries, K)
    try:
        if c["fill_first"]:
            # every counter of the batch filled by a run in which every column hits; the sparse runs below leave most of them stale
            batch.run(0.0, sparse_counts=True)
            check_hits(batch.hits(), us, ref, orders_of(us, ref, np.zeros_like(mks), False, ()), 10 ** 9, False, (name, "fill"))
        ran = 0
        for excluded in excluded_sets(sc, tie, ref[0], int(mks[0]), exact):
            orders = orders_of(us, ref, mks, exact, excluded)
            for limit in rc.stair_limits(sc, tie, ref[0], int(mks[0]), exact=exact, excluded=excluded):
                batch.set_limit(limit, excluded)
                batch.run(run_thr, sparse_counts=c["sparse"])
                if not c["devices"]:
                    inf = batch.info()
                    assert inf.exact == int(exact) and (exact or inf.count_bytes == c["route"]["count_bytes"])
                    nk, nu, mk = batch.unique()
                    assert np.array_equal(nu, us) and (exact or np.array_equal(mk, mks))
                check_hits(batch.hits(), us, ref, orders, limit, exact, (name, limit, excluded))
                ran += 1
        assert ran >= 8
        # without a limit again: the full lists
        batch.set_limit(None)
        batch.run(run_thr, sparse_counts=c["sparse"])
        check_hits(batch.hits(), us, ref, orders_of(us, ref, mks, exact, ()), 10 ** 9, exact, (name, "no limit"))
    finally:
        batch.close()
        st.delete_all()


def test_streamed_ranked_run_in_small_chunks(hip):
    """bigsi_hip_search_stream_ranked on the one-slice index, cut into chunks of a few queries: every chunk's batch runs the selection."""
    from bigsi_amd import _lib
    c, sc, queries, thr, tie = rc.build_stair("E_one_slice")
    us, ref = references("E_one_slice")
    mks = np.array([min_kmers(int(u), thr) for u in us], np.int64)
    st = open_index(c, sc)
    blob, soff = _lib.pack_seqs(queries)
    try:
        _lib.check(_lib.lib().bigsi_hip_stream_set_limits(st.handle, 2048, 4096, 100))
        for excluded in excluded_sets(sc, tie, ref[0], int(mks[0]), False):
            orders = orders_of(us, ref, mks, False, excluded)
            for limit in rc.stair_limits(sc, tie, ref[0], int(mks[0]), excluded=excluded)[::3]:
                nk, nu, off, col, cnt = st.search_many_packed(blob, soff, K, thr, limit=limit, excluded=list(excluded))
                assert np.array_equal(nu, us)
                check_hits((off, col, cnt), us, ref, orders, limit, False, ("stream", limit, excluded))
        n = _lib.C.c_uint64(0)
        _lib.lib().bigsi_hip_stream_last_chunks(st.handle, None, None, 0, _lib.C.byref(n))
        assert n.value >= 10          # (the stream was cut: 1024 queries in chunks of at most 100)
    finally:
        _lib.check(_lib.lib().bigsi_hip_stream_set_limits(st.handle, 0, 0, 0))
        st.delete_all()
