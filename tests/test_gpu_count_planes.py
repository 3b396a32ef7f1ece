"""The counting kernels behind every thresholded search -- k_and_count in its <P, H, CountT, KMX> instances, k_count_combine in both of
its code paths, the in-register counters of k_reads_fused -- bit for bit against numpy on a "staircase" index (tests/count_staircase.py)
whose per-column counts are chosen: 0, 1, u - 1, u, both sides of every power of two up to u (every carry of the ripple-carry adder
into every plane), and min_kmers - 1, min_kmers, min_kmers + 1 for thresholds whose min_kmers is a power of two and all ones below a
plane (every branch of the MSB-first comparator), at the first and last column of the first, second and last result word and of the
words at the tile cuts.  The rows go in with put_rows, every other row of the index is zero, and for the main query AND every filler
of the batch (substrings of the main query: varied counts from the same columns) unique(), counts() of all columns, the hit colours
and the hits' counts must equal the numpy reference.  Which route a case takes is pinned on the CPU against the compiled planner
(tests/test_count_staircase_host.py); here info() confirms the counter width and the one-launch route.

Case by case (count_staircase.CASES): S* one sliced query (k_count_combine: fast path up to 4 planes per slice, the loop beyond;
Smix: slices without k-mers; Sone: one slice); Uplain* one slice, 256 threads; Udeep* one-wavefront workgroups and the pipelined
loop; Usparse* hits only; Uearly the early exit against a wavefront whose columns become hits through their LAST k-mers only and sit
exactly on `need` at every check; Wide* 513 result words over five and two tiles; *_h1/2/5/7 the other H instances and the run-time-h
loop; R* the read kernel's three lane layouts."""
import itertools
import time

import numpy as np
import pytest

from count_staircase import CASES, K, build_case, min_kmers

pytestmark = pytest.mark.gpu
_counter = itertools.count()
_refs = {}


@pytest.fixture(scope="module")
def hip():
    import bigsi_amd
    from bigsi_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible"
    t0 = time.perf_counter()
    yield bigsi_amd
    print("test_gpu_count_planes wall time: %.1f s" % (time.perf_counter() - t0))


def references(name):
    """([u of every query], int32[n_queries, n_cols]): computed once per case, shared, never changed"""
    if name not in _refs:
        _, sc, queries = build_case(name)
        pairs = [sc.reference(q) for q in queries]
        _refs[name] = (np.array([u for u, _ in pairs], np.int64), np.stack([c for _, c in pairs]).astype(np.int32))
        _refs[name][1].setflags(write=False)
    return _refs[name]


def open_index(c, sc):
    from bigsi_amd.storage import get_storage
    st = get_storage({"storage-engine": "hip-hbm", "k": K, "m": c["m"], "h": c["h"],
                      "storage-config": {"name": "staircase%d" % next(_counter), "max_cols": c["n_cols"]}})
    st.delete_all()
    for key, v in (("number_of_rows", c["m"]), ("number_of_cols", c["n_cols"]), ("ksi:bloomfilter_size", c["m"]), ("ksi:num_hashes", c["h"])):
        st.set_integer(key, v)
    st.res.put_rows(sc.row_ids, sc.packed)
    return st


def check_run(c, batch, queries, us, ref, thr, what):
    """everything a run leaves, against numpy"""
    n = len(queries)
    inf = batch.info()
    assert inf.exact == 0 and inf.one_launch == c["one_launch"], what
    assert inf.count_bytes == (2 if c["one_launch"] else c["route"]["count_bytes"]), what
    nk, nu, mk = batch.unique()
    want_mk = np.array([min_kmers(int(u), thr) for u in us], np.int64)
    assert np.array_equal(nk, [max(len(q) - K + 1, 0) for q in queries]) and np.array_equal(nu, us) and np.array_equal(mk, want_mk), what
    off, col, cnt = batch.hits()
    qi, cols = np.nonzero(ref >= want_mk[:, None])          # (row-major: query by query, ascending colour)
    want_off = np.concatenate([[0], np.cumsum(np.bincount(qi, minlength=n))])
    bad = np.flatnonzero(np.diff(off.astype(np.int64)) != np.diff(want_off))
    assert bad.size == 0, (what, "hits per query", bad[:8], np.diff(off.astype(np.int64))[bad[:8]], np.diff(want_off)[bad[:8]])
    assert np.array_equal(col, cols), (what, "colours", qi[np.flatnonzero(col != cols)[:8]])
    assert np.array_equal(cnt, ref[qi, cols]), (what, "counts of hits", qi[np.flatnonzero(cnt != ref[qi, cols])[:8]])
    if not c["sparse"]:
        for i in range(n):
            got = batch.counts(i)
            assert np.array_equal(got, ref[i]), (what, "counts", i, np.flatnonzero(got != ref[i])[:8])
    return off, col, cnt


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_counts_and_hits_equal_numpy(hip, name):
    c, sc, queries = build_case(name)
    us, ref = references(name)
    st = open_index(c, sc)
    batch = st.new_batch(queries, K)
    try:
        for thr in sc.thresholds + [0.0]:           # (0.0: every valid column hits, the ragged last word masked)
            what = (name, thr)
            if c["early"]:
                # the same batch without the early exit first: the lists the flag must leave unchanged
                batch.run(thr, sparse_counts=True)
                plain = [x.copy() for x in check_run(c, batch, queries, us, ref, thr, what + ("no early exit",))]
            batch.run(thr, sparse_counts=c["sparse"], early_exit=c["early"])
            got = check_run(c, batch, queries, us, ref, thr, what)
            if c["early"]:
                assert all(np.array_equal(a, b) for a, b in zip(plain, got)), what
                if thr > 0.0:
                    # the column at min_kmers in the wavefront that may leave early is a hit of the main query
                    mk = min_kmers(sc.u, thr)
                    at_mk = [col for col, t, _ in sc.columns if col >= c["late_from"] and t == mk]
                    hits0 = got[1][int(got[0][0]):int(got[0][1])]
                    assert at_mk and set(at_mk) <= set(hits0.tolist()), what
    finally:
        batch.close()
        st.delete_all()
