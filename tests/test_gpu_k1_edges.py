"""The query front end (K1) on the device at its canonical-form and dedupe edges (tests/k1_cases.py; the cases are pinned on the CPU by
tests/test_k1_cases_host.py): k_kmerize_wave<31|0>, k_kmerize_lds<31|0> with one and eight workgroups per query, with its bytes
from memory, from the kernel arguments (1024 / 3072) or in place from pinned host memory, the four-kernel global route, K1 inside
k_reads_fused, and the build-side twins (k_bloom, k_insert_kmers), against a plain-Python reference.

Per run of a case the route first -- bigsi_hip_batch_last_row_and (k1_route, k1_parts, k1_arg_bytes, sorted_by, zero_copy) and
bigsi_hip_hits_last_path (one_launch) -- then the data, all of it exact: unique() (n, u, min_kmers), rows(), the first positions,
rep and pos_unique (bigsi_hip_batch_fetch_positions) of every query; where K1 sorted the row lists, the list K2 streamed as a
multiset and its bucket order.  The one-call routes expose no rows: they are held to their hits on an index planted from the
reference's rows, where a k-mer hashed on the wrong strand misses its column and a kernel that hits everything is caught by the
column that lacks one row."""
import itertools
import time

import numpy as np
import pytest

import k1_cases as kc
from k1_cases import CASES, K, ceil_thr, ref_of

pytestmark = pytest.mark.gpu
_counter = itertools.count()


@pytest.fixture(scope="module")
def hip():
    import bigsi_amd
    from bigsi_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible"
    t0 = time.perf_counter()
    yield bigsi_amd
    print("test_gpu_k1_edges wall time: %.1f s" % (time.perf_counter() - t0))


def open_index(k, h, m):
    from bigsi_amd.storage import get_storage
    st = get_storage({"storage-engine": "hip-hbm", "k": k, "m": m, "h": h, "storage-config": {"name": "k1edges%d" % next(_counter), "max_cols": kc.N_COLS}})
    st.delete_all()
    for key, v in (("number_of_rows", m), ("number_of_cols", kc.N_COLS), ("ksi:bloomfilter_size", m), ("ksi:num_hashes", h)):
        st.set_integer(key, v)
    return st


def last_route(owner, kind):
    from bigsi_amd import _lib
    out, hp = _lib.RowAndPath(), _lib.HitsPath()
    _lib.check(_lib.lib().bigsi_hip_batch_last_row_and(owner, kind, _lib.C.byref(out)))
    _lib.check(_lib.lib().bigsi_hip_hits_last_path(owner, kind, _lib.C.byref(hp)))
    got = {f: int(getattr(out, f)) for f, _ in _lib.RowAndPath._fields_}
    got["one_launch"] = int(hp.one_launch)
    return got


def check_route(want, got, what):
    assert got["one_launch"] == want["one_launch"], (what, got)
    if want["one_launch"]:
        # a read run reports the workgroups per query and the argument class, and leaves the rest of the record zero
        rest = {f: v for f, v in got.items() if f not in ("one_launch", "k1_parts", "k1_arg_bytes")}
        assert (got["k1_parts"], got["k1_arg_bytes"]) == (1, want["k1_arg_bytes"]) and not any(rest.values()), (what, got)
        return
    for f in ("k1_route", "k1_parts", "k1_arg_bytes", "sorted_by", "zero_copy"):
        assert got[f] == want[f], (what, f, got[f], want[f], got)


def check_data(c, batch, thr, what):
    """K1's outputs of every query of the batch against the reference"""
    from bigsi_amd import _lib
    k, h, m, queries = c["k"], c["h"], c["m"], c["queries"]
    refs = [ref_of(q, k) for q in queries]
    nk, nu, mk = batch.unique()
    assert nk.tolist() == [r.n for r in refs], (what, "num_kmers")
    assert nu.tolist() == [r.u for r in refs], (what, "num_unique", [(i, int(nu[i]), r.u) for i, r in enumerate(refs) if nu[i] != r.u][:5])
    assert mk.tolist() == [ceil_thr(r.u, thr) for r in refs], (what, "min_kmers")
    lookup = _lib.lib().bigsi_hip_batch_lookup
    first = np.zeros(max(max(r.u for r in refs), 1), np.uint32)
    for i, r in enumerate(refs):
        where = (what, "query %d of %d positions" % (i, r.n))
        rep, pu = batch.positions(i, r.n)
        assert rep.tolist() == r.rep, (where, "rep", [(p, int(rep[p]), r.rep[p]) for p in range(r.n) if rep[p] != r.rep[p]][:5])
        assert pu.tolist() == r.pos_unique, (where, "pos_unique")
        _lib.check(lookup(batch.b, i, _lib.ptr(first), None, first.size))            # (no row buffer: the first positions alone, one copy)
        assert first[:r.u].tolist() == r.first, (where, "first positions")
        rows = batch.rows(i, r.u).tolist()
        if rows != r.rows(h, m):
            t = next(t for t in range(r.u) if rows[t] != r.rows(h, m)[t])
            raise AssertionError("%s: rows of unique k-mer %d (%s at position %d, alignment %d, first difference %s): %s, wanted %s" % (
                where, t, r.uniq[t], r.first[t], r.first[t] & 3, kc.first_difference(r.uniq[t]), rows[t], r.rows(h, m)[t]))
    return refs


def check_sorted_lists(c, batch, refs, tab_mult, what):
    """the list K2 streamed, per query: the multiset of rows(), ascending in row >> shift for the shift of the query's own table"""
    from bigsi_amd import _lib
    fetch = _lib.lib().bigsi_hip_batch_fetch_rows_sorted
    h, m = c["h"], c["m"]
    cap = max(max(r.u for r in refs) * h, 1)
    got, shift = np.zeros(cap, np.uint64), _lib.C.c_uint32()
    for i, r in enumerate(refs):
        _lib.check(fetch(batch.b, i, _lib.ptr(got), cap, _lib.C.byref(shift)))
        slots, want_shift = kc.k1_table_slots(r.n, tab_mult), 0
        while m and ((m - 1) >> want_shift) >= slots:
            want_shift += 1
        assert shift.value == want_shift, (what, i, shift.value, want_shift)
        y = got[:r.u * h]
        assert sorted(y.tolist()) == sorted(x for kr in r.rows(h, m) for x in kr), (what, i, "the sorted list is not the multiset of the rows")
        assert not (np.diff((y >> np.uint64(want_shift)).astype(np.int64)) < 0).any(), (what, i, "the list steps down")


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_k1_outputs_equal_the_reference(hip, name):
    from bigsi_amd import _lib
    c = kc.CASE_BY_NAME[name]
    st = open_index(c["k"], c["h"], c["m"])
    try:
        batch = st.new_batch(c["queries"], c["k"])
        try:
            for (thr, kw), built_for in zip(c["runs"], c["built_for"]):
                what = (name, thr, kw, built_for)
                want = kc.expected_route(c["queries"], c["k"], c["h"], c["n_cols"], thr, kw)
                assert want["instance"] == built_for, what
                batch.run(thr, **kw)
                check_route(want, last_route(batch.b, _lib.HITS_PATH_OF_BATCH), what)
                refs = check_data(c, batch, thr, what)
                if want["sorted_by"] == kc.BY_K1:
                    check_sorted_lists(c, batch, refs, want["tab_mult"], what)
        finally:
            batch.close()
    finally:
        st.delete_all()


def test_one_call_searches_hit_the_planted_columns(hip):
    """search_batch with one sequence per call: the read kernel with its bytes in the arguments, k_kmerize_lds with 1024 or 3072
    bytes of arguments and reading pinned memory in place (eight workgroups per query from 256 positions on)"""
    from bigsi_amd import _lib
    pl = kc.planted("one_call")
    st = open_index(K, kc.H, kc.M)
    try:
        st.res.put_rows(*pl.packed())
        seen = set()
        for c, (cls, s) in enumerate(kc.ONE_CALL):
            for thr in (1.0, 0.5):
                what = (cls, c, len(s), thr)
                want = kc.expected_route([s], K, kc.H, kc.N_COLS, thr, dict(sparse_counts=True), one_call=True)
                nk, nu, off, col, cnt = st.search_batch_arrays([s], K, thr)
                check_route(want, last_route(st.handle, _lib.HITS_PATH_OF_INDEX), what)
                seen.add((cls, want["instance"], want["k1_arg_bytes"], want["k1_parts"]))
                n, u, mk, hit, counts = pl.expected(s, thr)
                assert (int(nk[0]), int(nu[0]), int(off[0]), int(off[1])) == (n, u, 0, len(hit)), (what, int(nk[0]), int(nu[0]), int(off[1]), len(hit))
                assert col.tolist() == hit, (what, "colours", sorted(set(col.tolist()) ^ set(hit))[:6], "column %d lacks row %d of unique k-mer %d" % ((c + 64,) + pl.dropped[c][::-1]))
                assert cnt.tolist() == counts, (what, "counts")
                if thr == 1.0:
                    assert c in hit and c + 64 not in hit
        assert seen == {("read", "k_reads_fused", 96, 1), ("arg1024", "k_kmerize_lds<31>", 1024, 1), ("arg1024", "k_kmerize_lds<31>", 1024, 8),
                        ("arg3072", "k_kmerize_lds<31>", 3072, 1), ("pinned", "k_kmerize_lds<31>", 0, 1)}, seen
    finally:
        st.delete_all()


def test_build_side_sets_exactly_the_rows_of_the_reference(hip):
    """k_bloom (BIGSI.bloom) and k_insert_kmers (insert_kmers) canonicalise byte-wise: every shape of set A and of every run-time k"""
    from bigsi_amd.graph.bigsi import BIGSI
    cfg = {"m": kc.M, "h": kc.H, "k": K}
    for k, shapes in [(K, kc.SHAPES)] + sorted(kc.RUNTIME_SHAPES.items()):
        st = open_index(k, kc.H, kc.M)
        try:
            for col, (key, s) in enumerate(shapes):
                want = sorted(set(kc.kmer_rows(s, kc.H, kc.M)))
                bits = np.unpackbits(np.frombuffer(BIGSI.bloom(cfg, [s]).tobytes(), np.uint8))[:kc.M]
                assert np.flatnonzero(bits).tolist() == want, (k, key, s, "bloom")
                st.insert_kmers(col, ["ACGT"[col % 4] * (col % 3) + s], k)          # (the shape is the last k-mer of a short sequence)
                extra = set(x for p in range(col % 3) for x in kc.kmer_rows(("ACGT"[col % 4] * (col % 3) + s)[p:p + k], kc.H, kc.M))
                bits = np.unpackbits(np.frombuffer(st.get_column(col), np.uint8))[:kc.M]
                assert np.flatnonzero(bits).tolist() == sorted(set(want) | extra), (k, key, s, "insert_kmers")
        finally:
            st.delete_all()
