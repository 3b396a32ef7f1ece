"""The exact row-AND -- k_and_exact<4|8> plain, sliced and in its chunked batch's re-planned tail, k_and_exact_band over windows and
segments, the exact instances of k_reads_fused -- and the two producers of the address-ordered row list in front of it (the fused
sort of k_kmerize_lds in both variants, k_sort_rows<256|1024>), bit for bit against numpy on a "knock-out" index
(tests/knockout_cases.py): every column but a few named edge columns holds every row of the main query EXCEPT ONE, so that a kernel
that SKIPS a row -- at a slice cut, in an unroll tail, at a window bound, in the second half of a split workgroup, through a lost
slot of a counting sort -- turns the column that knocks that row out into a hit.  (On random noise plus planted columns, the index of
the other exact tests, reading one row too few is invisible.)  The telling list positions are knocked first in every segment.

Per case: the route, asserted through bigsi_hip_batch_last_row_and and info() (pinned on the CPU against the compiled planner by
tests/test_knockout_host.py); unique(), hits() of every query and bitmap() of sampled ones against the numpy reference, every count
of an exact run being u; where the run made an address-ordered list, that list for every query -- the same multiset as rows(),
ascending in row >> shift, and for the main query the host's R; then one thresholded run on the same index at min_kmers = u - 1 of
the main query (a k-mer with one row knocked out must not count): colours and counts against numpy.  All comparisons are exact.  A
failure names the query, the column, the knocked row and where that row stands in the hash-order and the address-order list."""
import itertools
import time

import numpy as np
import pytest

import knockout_cases as kc
from knockout_cases import CASES, K, build_case, min_kmers, references, threshold_for

pytestmark = pytest.mark.gpu
_counter = itertools.count()
ROUTE_FIELDS = ("k1_route", "band_taken", "band_windows", "band_launches", "slices", "block", "tiles", "chunk_q", "n_launches", "last_slices",
                "last_block", "last_unroll", "sorted_by", "early_exit", "preset_by", "zero_copy")


@pytest.fixture(scope="module")
def hip():
    import bigsi_amd
    from bigsi_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible"
    t0 = time.perf_counter()
    yield bigsi_amd
    print("test_gpu_knockout wall time: %.1f s" % (time.perf_counter() - t0))


def open_index(c, ko):
    from bigsi_amd.storage import get_storage
    cfg = {"name": "knockout%d" % next(_counter), "max_cols": c["n_cols"]}
    if c["kind"] == "group":
        cfg["devices"] = c["devices"]
    st = get_storage({"storage-engine": "hip-hbm", "k": K, "m": c["m"], "h": c["h"], "storage-config": cfg})
    st.delete_all()
    for key, v in (("number_of_rows", c["m"]), ("number_of_cols", c["n_cols"]), ("ksi:bloomfilter_size", c["m"]), ("ksi:num_hashes", c["h"])):
        st.set_integer(key, v)
    st.res.put_rows(ko.row_ids, ko.packed)
    return st


def last_route(owner, kind):
    from bigsi_amd import _lib
    out = _lib.RowAndPath()
    _lib.check(_lib.lib().bigsi_hip_batch_last_row_and(owner, kind, _lib.C.byref(out)))
    return {f: int(getattr(out, f)) for f in ROUTE_FIELDS}


def check_route(c, got, n_seqs, what):
    want = c["route"]
    if want is None:                       # a one-launch read run leaves the record zero
        assert not any(got.values()), (what, got)
        return
    band = want["band"] or (0, 0)
    pairs = dict(k1_route=want["k1_route"], band_taken=int(bool(want["band"])), band_windows=band[0], band_launches=band[1],
                 slices=want["slices"], block=want["block"], tiles=want["tiles"], n_launches=want["n_launches"],
                 chunk_q=None if want["slices"] is None else (want["chunk_q"] or n_seqs), sorted_by=want["sorted_by"],
                 early_exit=want["early_exit"], preset_by=want["preset_by"], zero_copy=want["zero_copy"])
    if want["last"]:
        pairs.update(zip(("last_slices", "last_block", "last_unroll"), want["last"]))
    for key, v in pairs.items():
        assert v is None or got[key] == v, (what, key, got[key], v, got)


def check_lists(ko, queries, off, col, want_hit, what):
    """hit offsets and colours against the boolean matrix want_hit[n, n_cols]; the message says where the first difference lies"""
    n = len(queries)
    qi, cols = np.nonzero(want_hit)          # (row-major: query by query, ascending colour)
    want_off = np.concatenate([[0], np.cumsum(np.bincount(qi, minlength=n))])
    if np.array_equal(off.astype(np.int64), want_off) and np.array_equal(col, cols):
        return qi, cols
    for i in range(n):
        a, b = col[int(off[i]):int(off[i + 1])], cols[want_off[i]:want_off[i + 1]]
        if not np.array_equal(a, b):
            d = int(np.setxor1d(a, b)[0])
            raise AssertionError("%s: %s: %s (%d hits, %d wanted; differing columns %s)" % (
                what, "a column hits that must not" if d in a else "a hit is missing", ko.explain(i, queries[i], d), a.size, b.size,
                np.setxor1d(a, b)[:8].tolist()))
    raise AssertionError("%s: offsets differ" % (what,))


def check_exact(c, ko, queries, us, ref, nk, nu, mk, off, col, cnt, what):
    assert np.array_equal(nk, [max(len(q) - K + 1, 0) for q in queries]) and np.array_equal(nu, us) and np.array_equal(mk, us), what
    want_hit = (ref == us[:, None]) & (us[:, None] > 0)
    qi, _ = check_lists(ko, queries, off, col, want_hit, what)
    assert np.array_equal(cnt, us[qi]), (what, "every count of an exact run is u")
    return want_hit


def check_thresholded(ko, queries, us, ref, thr, nk, nu, mk, off, col, cnt, what):
    want_mk = np.array([min_kmers(int(u), thr) for u in us], np.int64)
    assert np.array_equal(nk, [max(len(q) - K + 1, 0) for q in queries]) and np.array_equal(nu, us) and np.array_equal(mk, want_mk), what
    qi, cols = check_lists(ko, queries, off, col, ref >= want_mk[:, None], what)
    bad = np.flatnonzero(cnt != ref[qi, cols])
    assert bad.size == 0, "%s: count %d, wanted %d: %s" % (what, cnt[bad[0]], ref[qi[bad[0]], cols[bad[0]]],
                                                          ko.explain(int(qi[bad[0]]), queries[qi[bad[0]]], int(cols[bad[0]])))


def sampled(n):
    return sorted(set(range(min(n, 12))) | set(np.random.default_rng(3).choice(n, size=min(n, 12), replace=False).tolist()))


def check_sorted_lists(c, ko, batch, queries, us, sorted_by, what):
    """the list K2 streamed, for every query: the multiset of rows(), ascending in row >> shift (the shift the producer must have
    used), and the main query's distinct rows are the host's R"""
    from bigsi_amd import _lib
    fetch, plain = _lib.lib().bigsi_hip_batch_fetch_rows_sorted, _lib.lib().bigsi_hip_batch_fetch_rows
    h, m, n = c["h"], c["m"], len(queries)
    tab_mult = 8 if n <= 32 else 4
    cap = max(int(us.max()) * h, 1)
    a, b, shift = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), _lib.C.c_uint32()
    pa, pb = _lib.ptr(a), _lib.ptr(b)
    for i in range(n):
        cnt = int(us[i]) * h
        _lib.check(plain(batch.b, i, pa, cap))
        _lib.check(fetch(batch.b, i, pb, cap, _lib.C.byref(shift)))
        pos = max(len(queries[i]) - K + 1, 0)
        want_shift = kc.sort_shift(m, kc.k1_table_slots(pos, tab_mult) if sorted_by == kc.BY_K1 else kc.SORT_BUCKETS)
        assert shift.value == want_shift, (what, i, shift.value, want_shift)
        x, y = a[:cnt], b[:cnt]
        if not np.array_equal(np.sort(x), np.sort(y)):
            lost = np.setdiff1d(x, y)
            extra = np.setdiff1d(y, x)
            raise AssertionError("%s: the sorted list of query %d is not the multiset of its rows: lost %s, extra or doubled %s; %s" % (
                what, i, lost[:4].tolist(), extra[:4].tolist(),
                ko.where(int(np.searchsorted(ko.R, lost[0]))) if lost.size else ""))
        down = np.flatnonzero(np.diff((y >> np.uint64(want_shift)).astype(np.int64)) < 0)
        assert down.size == 0, (what, "query %d: the list steps down at entry %d: rows %s, shift %d" % (i, down[0] + 1, y[down[0]:down[0] + 2].tolist(), want_shift))
        if i == 0:
            assert np.array_equal(np.unique(y), ko.R), (what, "R of the main query")
    err = fetch(batch.b, n, pb, cap, _lib.C.byref(shift))
    assert err == _lib.ERR_RANGE, (what, err)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_knockout_columns_do_not_hit(hip, name):
    from bigsi_amd import _lib
    c, ko, queries = build_case(name)
    us, ref = references(name)
    n = len(queries)
    st = open_index(c, ko)
    thr = threshold_for(int(us[0]), int(us[0]) - 1)
    try:
        if c["kind"] == "one_call":
            nk, nu, off, col, cnt = st.search_batch_arrays(queries, K, 1.0)
            check_route(c, last_route(st.handle, _lib.HITS_PATH_OF_INDEX), n, (name, "route"))
            check_exact(c, ko, queries, us, ref, nk, nu, nu, off, col, cnt, (name, "exact"))
            nk, nu, off, col, cnt = st.search_batch_arrays(queries, K, thr)
            check_thresholded(ko, queries, us, ref, thr, nk, nu, [min_kmers(int(u), thr) for u in us], off, col, cnt, (name, thr))
            return
        if c["limits"]:
            _lib.check(_lib.lib().bigsi_hip_band_set_limits(st.handle, *c["limits"]))
        batch = st.new_batch(queries, K)
        try:
            group = c["kind"] == "group"
            owner_kind = _lib.HITS_PATH_OF_GROUP_BATCH if group else _lib.HITS_PATH_OF_BATCH
            plain = None
            if c["run_kw"].get("early_exit"):
                # the same batch without the early exit first: the lists the flag must leave unchanged
                batch.run(1.0)
                assert last_route(batch.b, owner_kind)["early_exit"] == 0
                plain = [x.copy() for x in batch.hits()]
            batch.run(1.0, **c["run_kw"])
            got = last_route(batch.b, owner_kind)
            check_route(c, got, n, (name, "route"))
            if not group:
                inf = batch.info()
                assert inf.exact == 1 and inf.one_launch == int(c["kind"] == "reads"), (name, inf.exact, inf.one_launch)
            nk, nu, mk = batch.unique()
            off, col, cnt = batch.hits()
            want_hit = check_exact(c, ko, queries, us, ref, nk, nu, mk, off, col, cnt, (name, "exact"))
            if plain is not None:
                assert all(np.array_equal(x, y) for x, y in zip(plain, (off, col, cnt))), (name, "the early exit changed the lists")
            if not group:
                for i in sampled(n):
                    bm = batch.bitmap(i)
                    want = np.packbits(want_hit[i])
                    bad = np.flatnonzero(bm[:want.size] != want)
                    assert bad.size == 0 and not bm[want.size:].any(), "%s: bitmap: %s" % (
                        name, ko.explain(i, queries[i], int(np.flatnonzero(np.unpackbits(bm[:want.size] ^ want)[:c["n_cols"]])[0])) if bad.size else "bits behind the last column")
                if got["sorted_by"] != kc.NONE:
                    check_sorted_lists(c, ko, batch, queries, us, got["sorted_by"], (name, "sorted list"))
                else:
                    shift = _lib.C.c_uint32()
                    rows = np.zeros(max(int(us.max()) * c["h"], 1), np.uint64)
                    assert _lib.lib().bigsi_hip_batch_fetch_rows_sorted(batch.b, 0, _lib.ptr(rows), rows.size, _lib.C.byref(shift)) == _lib.ERR_STATE
            # the counting kernels on the same index: a k-mer with one row knocked out must not count
            batch.run(thr, sparse_counts=c["kind"] == "reads")
            if not group:
                inf = batch.info()
                assert inf.exact == 0 and inf.one_launch == int(c["kind"] == "reads"), (name, thr)
            nk, nu, mk = batch.unique()
            off, col, cnt = batch.hits()
            check_thresholded(ko, queries, us, ref, thr, nk, nu, mk, off, col, cnt, (name, thr))
            if c["kind"] == "batch":
                for i in sampled(n)[:6]:
                    counts = batch.counts(i)
                    bad = np.flatnonzero(counts != ref[i])
                    assert bad.size == 0, "%s: counts: %d, wanted %d: %s" % (name, counts[bad[0]], ref[i][bad[0]], ko.explain(i, queries[i], int(bad[0])))
        finally:
            batch.close()
    finally:
        if c["limits"]:
            _lib.check(_lib.lib().bigsi_hip_band_set_limits(st.handle, 0, 0))
        st.delete_all()
