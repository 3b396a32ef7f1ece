"""The code every search ends in -- K4's k_hits_totals / k_hits_write in both bodies, the export into pinned host memory (inline in
k_hits_write or the read kernel, k_export_results, k_export_reads) and bigsi_batch_collect -- bit for bit against numpy on indexes
whose hit lists are chosen (tests/hits_cases.py): empty lists, every column, the first and the last column alone, the last column of
one word with the first of the next at every thread, chunk, group and shard cut, one hit per word, totals of exactly 1023 / 1024 /
1025 (the export's size) and 65 535 / 65 536 / 65 537 (the lists' capacity) with a small call through the grown workspace behind
them, the regrow + write-only pass of a batch, read runs either side of exp_spec, a device group of uneven shards.  Every call first
asserts, through bigsi_hip_hits_last_path, the path it was built for -- a case that silently takes another path fails -- and then
compares unique(), the hit offsets, colours and counts (exact: one-k-mer queries; thresholded at 0.5: two-k-mer queries, counts 1 or
2 by column).  Which path a case takes is pinned on the CPU against the compiled planner (tests/test_hits_cases_host.py).  Everything
is integer: no tolerances.  Needs a real MI355X: `pytest -m gpu`."""
import itertools

import numpy as np
import pytest

import hits_cases as hc
from hits_cases import K, build_case

pytestmark = pytest.mark.gpu
GUARD, GUARD_WORD = 16, 0xA5A5A5A5
PATH_FIELDS = ("groups", "items_per_group", "single_workgroup", "inline_export", "rewrites", "exp_spec", "collect_fetch", "one_launch")
_counter = itertools.count()


@pytest.fixture(scope="module")
def hip():
    import bigsi_amd
    from bigsi_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible"
    return bigsi_amd


def open_index(b):
    from bigsi_amd.storage import get_storage
    c = b.case
    cfg = {"name": "hits%d" % next(_counter), "max_cols": c["n_cols"]}
    if c["devices"]:
        cfg["devices"] = c["devices"]
    st = get_storage({"storage-engine": "hip-hbm", "k": K, "m": b.m, "h": c["h"], "storage-config": cfg})
    st.delete_all()
    for key, v in (("number_of_rows", b.m), ("number_of_cols", c["n_cols"]), ("ksi:bloomfilter_size", b.m), ("ksi:num_hashes", c["h"])):
        st.set_integer(key, v)
    st.res.put_rows(b.row_ids, b.packed)
    return st


def last_path(owner, kind):
    from bigsi_amd import _lib
    out = _lib.HitsPath()
    _lib.check(_lib.lib().bigsi_hip_hits_last_path(owner, kind, _lib.C.byref(out)))
    return {f: int(getattr(out, f)) for f in PATH_FIELDS}


def one_call(st, seqs, threshold, cap):
    """bigsi_hip_search_batch by hand: (nk, nu, mk, off, col, cnt); the lists carry GUARD words behind their capacity"""
    from bigsi_amd import _lib
    blob, soff = _lib.pack_seqs(seqs)
    n = len(seqs)
    nk, nu, mk = (np.full(n, 0xDEAD, np.uint32) for _ in range(3))
    off = np.full(n + 1, 0xDEAD, np.uint64)
    col, cnt = np.full(cap + GUARD, GUARD_WORD, np.uint32), np.full(cap + GUARD, GUARD_WORD, np.uint32)
    _lib.check(_lib.lib().bigsi_hip_search_batch(st.handle, blob, _lib.ptr(soff), n, K, float(threshold), 0, _lib.ptr(nk), _lib.ptr(nu), _lib.ptr(mk),
                                                 _lib.ptr(off), _lib.ptr(col), _lib.ptr(cnt), cap))
    assert (col[cap:] == GUARD_WORD).all() and (cnt[cap:] == GUARD_WORD).all(), "the call wrote behind its capacity"
    total = int(off[-1])
    assert (col[total:] == GUARD_WORD).all() and (cnt[total:] == GUARD_WORD).all(), "the call wrote behind its total"
    return nk, nu, mk, off, col[:total], cnt[:total]


def assert_results(got, want, what):
    for label, g, w in zip(("num_kmers", "num_unique", "min_kmers", "hit offsets"), got[:4], want[:4]):
        assert np.array_equal(g, w), (what, label, np.flatnonzero(np.asarray(g) != np.asarray(w))[:8])
    for label, g, w in zip(("colours", "counts"), got[4:], want[4:]):
        assert g.size == w.size, (what, label, g.size, w.size)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, label, bad[:8], g[bad[:8]], w[bad[:8]])


@pytest.mark.parametrize("name,mode", hc.PARAMS)
def test_hit_lists_equal_numpy(hip, name, mode):
    from bigsi_amd import _lib
    b = build_case(name, mode)
    c, thr = b.case, b.threshold
    paths = [{f: p[f] for f in PATH_FIELDS} for p in b.paths()]
    st = open_index(b)
    try:
        for i, (call, want_path) in enumerate(zip(b.calls, paths)):
            seqs, want, what = [b.queries[q] for q in call], b.expected(call), (name, mode, i, [b.patterns[q] for q in call][:4])
            if c["kind"] in ("one_call", "reads"):
                got = one_call(st, seqs, thr, int(want[3][-1]) + 1)
                assert last_path(st.handle, _lib.HITS_PATH_OF_INDEX) == want_path, what
                assert_results(got, want, what)
                # ... and what the binding makes of the same call
                res = st.search_batch(seqs, K, thr)
                assert [(r[0], r[1]) for r in res] == list(zip(want[0].tolist(), want[1].tolist())), what
                off = want[3].astype(np.int64)
                for j, r in enumerate(res):
                    assert np.array_equal(r[2], want[4][off[j]:off[j + 1]]) and np.array_equal(r[3], want[5][off[j]:off[j + 1]]), what + (j,)
            else:
                batch = st.new_batch(seqs, K)
                try:
                    batch.run(thr, **c["run_kw"])
                    nk, nu, mk = batch.unique()
                    off, col, cnt = batch.hits()
                    kind = _lib.HITS_PATH_OF_GROUP_BATCH if c["kind"] == "group" else _lib.HITS_PATH_OF_BATCH
                    assert last_path(batch.b, kind) == want_path, what
                    assert_results((nk, nu, mk, off, col, cnt), want, what)
                    # a second fetch finds the lists as the first left them (after a regrow: the rewritten ones)
                    off2, col2, cnt2 = batch.hits()
                    assert last_path(batch.b, kind) == want_path, what
                    assert_results((nk, nu, mk, off2, col2, cnt2), want, what)
                finally:
                    batch.close()
    finally:
        st.delete_all()


def test_the_hook_reports_nothing_before_a_run(hip):
    """STATE for a batch that has not run and for an index whose one-call workspace does not exist yet; INVALID for an unknown kind"""
    from bigsi_amd import _lib
    b = build_case("one_100", "exact")
    st = open_index(b)
    try:
        out, fn = _lib.HitsPath(), _lib.lib().bigsi_hip_hits_last_path
        assert fn(st.handle, _lib.HITS_PATH_OF_INDEX, _lib.C.byref(out)) == _lib.ERR_STATE
        batch = st.new_batch(b.queries[:2], K)
        try:
            assert fn(batch.b, _lib.HITS_PATH_OF_BATCH, _lib.C.byref(out)) == _lib.ERR_STATE
            assert fn(batch.b, 7, _lib.C.byref(out)) == _lib.ERR_INVALID and fn(batch.b, _lib.HITS_PATH_OF_BATCH, None) == _lib.ERR_INVALID
            batch.run(1.0)
            assert last_path(batch.b, _lib.HITS_PATH_OF_BATCH) == dict(groups=1, items_per_group=2, single_workgroup=1, inline_export=0, rewrites=0,
                                                                       exp_spec=0, collect_fetch=0, one_launch=0)
            # a run without hit lists reports no K4
            batch.run(1.0, skip_compact=True)
            assert last_path(batch.b, _lib.HITS_PATH_OF_BATCH)["groups"] == 0
        finally:
            batch.close()
    finally:
        st.delete_all()
