"""The band sweep of the exact row-AND (k_and_exact_band, plan_band_sweep): one column segment of EVERY query per launch, a band cut
into address windows, the accumulator carried from window to window in the result words.  Forced here with BIGSI_RUN_BAND_SWEEP on a
small index -- m = 1009 rows, h = 3, k = 31 -- at two widths: 8261 columns = 130 result words (two segments, the second held by ONE
lane) and 8253 columns = 129 words (the last lane's second word is past the end).  301 queries (not a multiple of 8) of 100 bp, six of
them planted in samples, two identical ones (shared rows by construction), one shorter than k and one of exactly k.  Hit lists and
bitmaps must equal the default route's on the same batch, and sampled queries the oracle's.  Needs a real MI355X: `pytest -m gpu`."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, H, K = 1009, 3, 31
N_QUERIES = 301
WIDTHS = (8261, 8253)
WINDOWS = (1, 3, 16, 2000)          # 2000: more windows than rows, most of them empty
SEGS = (1, 2)
SAMPLED = (0, 1, 5, 17, 100, 200, 297, 298, 299, 300)
_names = itertools.count()


def random_seqs(rng, n, length):
    return ["".join(rng.choice(list("ACGT"), size=length)) for _ in range(n)]


def make_queries():
    base = random_seqs(np.random.default_rng(31), 298, 100)
    seqs = base + [base[0], base[2][:K - 1], base[3][:K]]          # 298: a copy of query 0; 299: no k-mer; 300: one k-mer
    assert len(seqs) == N_QUERIES
    return seqs


def plants(n_cols):
    """(column, query): both ends of the row, both sides of the segment boundary at column 8192, the last lane's words"""
    return ((0, 0), (100, 0), (5000, 0), (n_cols - 1, 0), (8192, 5), (8191, 17), (n_cols - 2, 100), (64, 200), (8200, 297), (63, 300))


def new_index(n_cols, seed, max_cols=None):
    from bigsi_amd.storage import get_storage
    st = get_storage({"storage-engine": "hip-hbm", "storage-config": {"name": "band%d" % next(_names), "max_cols": max_cols or n_cols},
                      "k": K, "m": M, "h": H})
    st.delete_all()
    st.set_integer("number_of_rows", M)
    st.set_integer("number_of_cols", n_cols)
    st.set_integer("ksi:bloomfilter_size", M)
    st.set_integer("ksi:num_hashes", H)
    st.fill_synthetic(seed, 0, 1)
    return st


def launches(st):
    from bigsi_amd import _lib
    s = _lib.Stats()
    _lib.check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(s), 0))
    return int(s.and_launches_total)


def set_limits(st, windows, segs):
    from bigsi_amd import _lib
    _lib.check(_lib.lib().bigsi_hip_band_set_limits(st.handle, windows, segs))


class Case(object):
    """An index of one width, the batch, and the default route's answers (computed once, never changed)."""

    def __init__(self, n_cols):
        from bigsi_amd import _lib
        from oracle.ref_model import SynthOracle
        assert _lib.device_count() >= 1, "no HIP device visible"
        self.n_cols, self.seqs = n_cols, make_queries()
        self.st = new_index(n_cols, 77)
        self.orc = SynthOracle(77, 0, M, n_cols, H, K, 1)
        for col, q in plants(n_cols):
            self.st.insert_kmers(col, [self.seqs[q]], K)
            self.orc.insert_kmers(col, self.seqs[q])
        self.batch = self.st.new_batch(self.seqs, K)
        before = launches(self.st)
        self.batch.run(1.0)
        self.default_launches = launches(self.st) - before
        self.hits = [x.copy() for x in self.batch.hits()]
        self.bitmaps = {i: self.batch.bitmap(i).copy() for i in SAMPLED}
        self.nu = self.batch.unique()[1].copy()

    def same_as_default(self, what):
        for a, b in zip(self.hits, self.batch.hits()):
            assert np.array_equal(a, b), what
        for i in SAMPLED:
            assert np.array_equal(self.batch.bitmap(i), self.bitmaps[i]), (what, i)

    def forced(self, windows, segs, **kw):
        """one forced run; returns the row-AND launches it made"""
        set_limits(self.st, windows, segs)
        before = launches(self.st)
        self.batch.run(1.0, band_sweep=True, **kw)
        n = launches(self.st) - before
        set_limits(self.st, 0, 0)
        return n

    def close(self):
        self.batch.close()
        self.st.delete_all()


@pytest.fixture(scope="module", params=WIDTHS)
def case(request):
    c = Case(request.param)
    yield c
    c.close()


def test_default_route_matches_the_oracle(case):
    """The reference of every other test here: the default route (a sliced launch: 602 wavefronts) against SynthOracle on the sampled
    queries, the planted columns among the hits, no hit for the query without k-mers."""
    off, col, cnt = case.hits
    assert case.default_launches == 1
    for i in SAMPLED:
        if len(case.seqs[i]) < K:
            continue
        u, want_cnt = case.orc.counts(case.seqs[i])
        want = np.flatnonzero(want_cnt >= u)
        assert case.nu[i] == u, i
        assert np.array_equal(col[int(off[i]):int(off[i + 1])], want), i
        assert np.array_equal(cnt[int(off[i]):int(off[i + 1])], want_cnt[want].astype(np.uint32)), i
    assert case.nu[299] == 0 and off[299] == off[300] and case.nu[300] == 1
    for c, q in plants(case.n_cols):
        assert c in col[int(off[q]):int(off[q + 1])].tolist(), (c, q)
    assert np.array_equal(col[int(off[0]):int(off[1])], col[int(off[298]):int(off[299])])          # the identical pair


@pytest.mark.parametrize("windows,segs", list(itertools.product(WINDOWS, SEGS)))
def test_forced_band_sweep_equals_default_route(case, windows, segs):
    n = case.forced(windows, segs)
    assert n == -(-2 // segs) * windows                    # the route was taken: bands x windows launches
    case.same_as_default((windows, segs))


def test_planner_values_when_nothing_is_forced(case):
    """0 keeps the planner's own windows and segments: 301 queries are one window, and the second segment's one or two words ride in
    the first segment's launch -- one launch of two segments."""
    assert case.forced(0, 0) == 1
    case.same_as_default("planner's own")


def test_same_batch_again_after_other_queries(case):
    """The first window starts from all ones, not from the words the run before left: the batch object runs OTHER queries through the
    route (their results then lie in the result words), then the first set again."""
    other = random_seqs(np.random.default_rng(32), N_QUERIES, 100)
    case.batch.reload(other, K)
    assert case.forced(3, 1) == 6
    case.batch.reload(case.seqs, K)
    assert case.forced(3, 1) == 6
    case.same_as_default("after other queries")
    assert case.forced(16, 2) == 16                        # and twice in a row
    case.same_as_default("twice in a row")


def test_limit(case):
    case.batch.set_limit(3)
    try:
        case.batch.run(1.0)
        want = [x.copy() for x in case.batch.hits()]
        assert int(np.diff(want[0].astype(np.int64)).max()) == 3
        assert case.forced(3, 2) == 3
        for a, b in zip(want, case.batch.hits()):
            assert np.array_equal(a, b)
    finally:
        case.batch.set_limit(0)
    case.batch.run(1.0)
    case.same_as_default("limit off again")


def test_early_exit_declines_the_route(case):
    """BIGSI_RUN_EARLY_EXIT together with the force flag: the route declines (the default plan's single launch) and results match."""
    assert case.forced(3, 1, early_exit=True) == case.default_launches
    case.same_as_default("early exit")


def test_caller_owned_outputs_of_another_stride():
    """bigsi_hip_batch_set_outputs with a wider result_cols: the result words of a query lie result-width apart, not index-width.
    The whole caller-owned buffer must equal the default route's, word for word (words behind the index's own columns included)."""
    import torch
    from bigsi_amd import _lib
    n_cols, result_cols = 8261, 8261 + 300
    st = new_index(n_cols, 78, max_cols=n_cols + 512)
    seqs = make_queries()
    for col, q in plants(n_cols):
        st.insert_kmers(col, [seqs[q]], K)
    L = _lib.lib()
    b = st.new_batch(seqs, K)
    _lib.check(L.bigsi_hip_batch_set_result_cols(b.b, result_cols))
    stride = (-(-result_cols // 64) + 1) // 2 * 2 * 8
    assert stride != (-(-n_cols // 64) + 1) // 2 * 2 * 8
    bufs = []
    for force in (False, True, True):
        buf = torch.full((len(seqs) * stride,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.bigsi_hip_batch_set_outputs(b.b, buf.data_ptr()))
        if force:
            set_limits(st, 3 if len(bufs) == 1 else 16, len(bufs))
        before = launches(st)
        b.run(1.0, skip_compact=True, band_sweep=force)
        _lib.check(L.bigsi_hip_synchronize(st.handle))
        assert launches(st) - before == (1 if not force else 6 if len(bufs) == 1 else 16)
        bufs.append(buf.cpu().numpy().reshape(len(seqs), stride))
    set_limits(st, 0, 0)
    words = -(-result_cols // 64) * 8
    for got in bufs[1:]:
        assert np.array_equal(got[:, :words], bufs[0][:, :words])
    assert bufs[0][5, :words].any() and not bufs[0][299, :words].any()          # a planted query, the one without k-mers
    b.close()
    st.delete_all()
