"""The streamed search (bigsi_hip_search_stream, _ranked, _scored: search_stream_impl) at its chunk cuts, on small inputs: the limits
are set through bigsi_hip_stream_set_limits so that a few hundred short queries make many chunks, the cuts are read back with
bigsi_hip_stream_last_chunks and must equal the restatement of the rule in tests/stream_ref.py -- every test asserts the cuts it
relies on first.  Results never depend on the cuts: they are compared with the oracle (first and last query, two queries either side
of every cut, every 7th of the rest) and, whole, with plain batch runs cut elsewhere.  A synthetic index of m = 1009 rows, h = 3,
k = 31 at two widths: 8261 columns (130 result words, two band segments) and 333 (a partial last word).  The C ABI is called directly
through bigsi_amd._lib.  Needs a real MI355X: `pytest -m gpu`."""
import collections
import itertools

import numpy as np
import pytest

import stream_ref

pytestmark = pytest.mark.gpu

M, H, K = 1009, 3, 31
WIDE, NARROW = 8261, 333
GUARD, GUARD_WORD, GUARD_BYTE = 16, 0xA5A5A5A5, 0x5A
_names = itertools.count()

Out = collections.namedtuple("Out", "rc nk nu mk off col cnt")
Scored = collections.namedtuple("Scored", "rc nk nu mk off col cnt bits boff rec need")


def rand_seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode("ascii")


def random_seqs(rng, n, length):
    return [rand_seq(rng, length) for _ in range(n)]


def memoised_oracle(*args):
    """SynthOracle with its rows kept: the index has 1009 of them and a test reads each hundreds of times"""
    from oracle.ref_model import SynthOracle

    class Memoised(SynthOracle):
        kept = {}

        def row(self, r):
            if r not in self.kept:
                self.kept[r] = SynthOracle.row(self, r)
            return self.kept[r].copy()

        def insert_kmers(self, colour, seq):
            SynthOracle.insert_kmers(self, colour, seq)
            self.kept.clear()

    orc = Memoised(*args)
    orc.kept = {}
    return orc


class Case(object):
    """An index of one width with its oracle; plant() adds a sequence's k-mers to a column on both sides."""

    def __init__(self, n_cols, seed):
        from bigsi_amd import _lib
        from bigsi_amd.storage import get_storage
        assert _lib.device_count() >= 1, "no HIP device visible"
        self.n_cols = n_cols
        self.st = get_storage({"storage-engine": "hip-hbm", "storage-config": {"name": "cuts%d" % next(_names), "max_cols": n_cols}, "k": K, "m": M, "h": H})
        self.st.delete_all()
        for key, v in (("number_of_rows", M), ("number_of_cols", n_cols), ("ksi:bloomfilter_size", M), ("ksi:num_hashes", H)):
            self.st.set_integer(key, v)
        self.st.fill_synthetic(seed, 0, 1)
        self.orc = memoised_oracle(seed, 0, M, n_cols, H, K, 1)
        self._oracle_cache = {}

    def plant(self, col, seq):
        self.st.insert_kmers(col, [seq], K)
        self.orc.insert_kmers(col, seq)
        self._oracle_cache.clear()

    def counts(self, seq):
        if seq not in self._oracle_cache:
            self._oracle_cache[seq] = self.orc.counts(seq)
        return self._oracle_cache[seq]

    def close(self):
        set_limits(self.st, 0, 0, 0)
        self.st.delete_all()


@pytest.fixture(scope="module", params=[WIDE, NARROW])
def case(request):
    c = Case(request.param, 91)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide():
    c = Case(WIDE, 92)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ the two test entry points
def set_limits(st, chunk_positions, large_chunk_positions, chunk_seqs):
    from bigsi_amd import _lib
    _lib.check(_lib.lib().bigsi_hip_stream_set_limits(st.handle, chunk_positions, large_chunk_positions, chunk_seqs))


def last_chunks(st):
    """[(first sequence, band)] of the last stream call: the sizing call, then the fetch"""
    from bigsi_amd import _lib
    n = _lib.C.c_uint64(0)
    rc = _lib.lib().bigsi_hip_stream_last_chunks(st.handle, None, None, 0, _lib.C.byref(n))
    if n.value == 0:
        assert rc == _lib.OK
        return []
    assert rc == _lib.ERR_CAPACITY
    first, band = np.full(n.value + 1, 0xFFFF, np.uint64), np.full(n.value + 1, 0x77, np.uint8)
    _lib.check(_lib.lib().bigsi_hip_stream_last_chunks(st.handle, _lib.ptr(first), _lib.ptr(band), n.value, _lib.C.byref(n)))
    assert first[-1] == 0xFFFF and band[-1] == 0x77 and n.value == first.size - 1
    return [(int(f), bool(b)) for f, b in zip(first[:-1], band[:-1])]


def expected_cuts(case, seqs, threshold, limits, **kw):
    """the restatement's chunks for these limits; asserts that the last call cut there and returns [(first, band, n, max_pos)]"""
    want = stream_ref.cuts([len(s) for s in seqs], K, threshold, case.n_cols, H, M, chunk_positions=limits[0], large_chunk_positions=limits[1],
                           chunk_seqs=limits[2], **kw)
    assert last_chunks(case.st) == [(f, b) for f, b, _, _ in want]
    return want


# ------------------------------------------------------------------------------------------------ the three streams, by hand
def guarded(n, dtype, fill):
    return np.full(n + GUARD, fill, dtype)


def stream(st, seqs, threshold, flags=0, cap=None, limit=0, excluded=None, packed=None):
    """bigsi_hip_search_stream (or _ranked with a limit).  cap = None: the sizing call (capacity 0, NULL lists), then the call with
    exactly what it reported -- both must leave the same offsets.  The lists carry GUARD words behind their capacity."""
    from bigsi_amd import _lib
    L = _lib.lib()
    blob, soff = packed if packed is not None else _lib.pack_seqs(seqs)
    n = len(soff) - 1
    ex = np.ascontiguousarray(excluded if excluded is not None else [], dtype=np.uint32)

    def call(cap_, col, cnt, nk, nu, mk, off):
        head = (st.handle, blob, _lib.ptr(soff), n, K, float(threshold), flags, _lib.ptr(nk), _lib.ptr(nu), _lib.ptr(mk), _lib.ptr(off),
                _lib.ptr(col), _lib.ptr(cnt), cap_)
        if limit:
            return L.bigsi_hip_search_stream_ranked(*head, limit, _lib.ptr(ex) if ex.size else None, ex.size)
        return L.bigsi_hip_search_stream(*head)

    sized = None
    if cap is None:
        sized = np.full(n + 1, 0xDEAD, np.uint64)
        rc = call(0, None, None, None, None, None, sized)
        assert rc in (_lib.OK, _lib.ERR_CAPACITY) and (rc == _lib.OK) == (int(sized[-1]) == 0), rc
        cap = int(sized[-1])
    nk, nu, mk, off = np.full(n, 0xDEAD, np.uint32), np.full(n, 0xDEAD, np.uint32), np.full(n, 0xDEAD, np.uint32), np.full(n + 1, 0xDEAD, np.uint64)
    col, cnt = guarded(cap, np.uint32, GUARD_WORD), guarded(cap, np.uint32, GUARD_WORD)
    rc = call(cap, col, cnt, nk, nu, mk, off)
    assert (col[cap:] == GUARD_WORD).all() and (cnt[cap:] == GUARD_WORD).all(), "the stream wrote behind its capacity"
    if sized is not None:
        assert rc == _lib.OK and np.array_equal(sized, off)
    return Out(rc, nk, nu, mk, off, col[:cap], cnt[:cap])


def stream_scored(st, seqs, threshold, cap, bits_cap, flags=0):
    from bigsi_amd import _lib
    from bigsi_amd.scoring import HIT_SCORE_DTYPE
    blob, soff = _lib.pack_seqs(seqs)
    n = len(seqs)
    nk, nu, mk, off = np.full(n, 0xDEAD, np.uint32), np.full(n, 0xDEAD, np.uint32), np.full(n, 0xDEAD, np.uint32), np.full(n + 1, 0xDEAD, np.uint64)
    col, cnt = guarded(cap, np.uint32, GUARD_WORD), guarded(cap, np.uint32, GUARD_WORD)
    bits, boff, rec = guarded(bits_cap, np.uint8, GUARD_BYTE), np.zeros(cap + 1, np.uint64), np.zeros(max(cap, 1), HIT_SCORE_DTYPE)
    need = np.full(1, 0xDEAD, np.uint64)
    rc = _lib.lib().bigsi_hip_search_stream_scored(st.handle, blob, _lib.ptr(soff), n, K, float(threshold), flags, _lib.ptr(nk), _lib.ptr(nu), _lib.ptr(mk),
                                                   _lib.ptr(off), _lib.ptr(col), _lib.ptr(cnt), cap, _lib.ptr(bits), bits_cap, _lib.ptr(boff),
                                                   _lib.ptr(rec), _lib.ptr(need))
    assert (col[cap:] == GUARD_WORD).all() and (cnt[cap:] == GUARD_WORD).all() and (bits[bits_cap:] == GUARD_BYTE).all(), "the stream wrote behind its capacity"
    return Scored(rc, nk, nu, mk, off, col[:cap], cnt[:cap], bits[:bits_cap], boff, rec[:cap], int(need[0]))


# ------------------------------------------------------------------------------------------------ the references
def checked_indices(n, firsts):
    """first and last query, two either side of every cut, every 7th of the rest"""
    idx = {0, n - 1} | set(range(0, n, 7))
    for f in firsts:
        idx |= {i for i in (f - 2, f - 1, f, f + 1) if 0 <= i < n}
    return sorted(idx)


def assert_oracle(case, seqs, threshold, out, firsts, indices=None):
    checked = 0
    for i in (indices if indices is not None else checked_indices(len(seqs), firsts)):
        u, want_cnt = case.counts(seqs[i])
        assert out.nk[i] == max(len(seqs[i]) - K + 1, 0) and out.nu[i] == u, i
        lo, hi = int(out.off[i]), int(out.off[i + 1])
        if u == 0:          # no k-mer: the reference raises; exact -> no hit, thresholded -> every column with count 0 (0 >= ceil(0 * t))
            assert (hi - lo) == (0 if threshold == 1.0 else case.n_cols) and not out.cnt[lo:hi].any(), i
            continue
        mk = int(np.ceil(u * threshold))
        assert out.mk[i] == mk, i
        want = np.flatnonzero(want_cnt >= (u if threshold == 1.0 else mk))
        assert np.array_equal(out.col[lo:hi], want), (threshold, i)
        assert np.array_equal(out.cnt[lo:hi], want_cnt[want].astype(np.uint32)), (threshold, i)
        checked += 1
    return checked


def batch_step(n, firsts):
    """a batch size whose multiples are not the stream's cuts"""
    for step in (97, 89, 101, 53, 113, 61, 37):
        if not set(range(step, n, step)) & set(firsts):
            return step
    raise AssertionError("no batch size avoids the cuts %r" % (firsts,))


def assert_equals_batches(case, seqs, threshold, out, firsts, limit=0, excluded=None, **run_kw):
    """the whole output against plain batch runs cut elsewhere"""
    step = batch_step(len(seqs), firsts)
    for lo in range(0, len(seqs), step):
        part = seqs[lo:lo + step]
        b = case.st.new_batch(part, K)
        if limit:
            b.set_limit(limit, excluded)
        b.run(threshold, sparse_counts=True, **run_kw)
        bnk, bnu, bmk = b.unique()
        boff, bcol, bcnt = b.hits()
        b.close()
        hi = lo + len(part)
        assert np.array_equal(out.nk[lo:hi], bnk) and np.array_equal(out.nu[lo:hi], bnu) and np.array_equal(out.mk[lo:hi], bmk), lo
        assert np.array_equal(out.off[lo:hi + 1].astype(np.int64) - int(out.off[lo]), boff.astype(np.int64)), lo
        assert np.array_equal(out.col[int(out.off[lo]):int(out.off[hi])], bcol) and np.array_equal(out.cnt[int(out.off[lo]):int(out.off[hi])], bcnt), lo


def assert_same(a, b):
    for name in ("nk", "nu", "mk", "off", "col", "cnt"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def plant_around(case, seqs, firsts, base=3):
    """a hit in the last query before every cut and in the first behind it, in columns spread over the width (the last one included)"""
    planted = []
    for j, f in enumerate(firsts):
        for i in (f - 1, f):
            if 0 <= i < len(seqs) and len(seqs[i]) >= K:
                col = (base + 997 * len(planted)) % case.n_cols if planted else case.n_cols - 1
                case.plant(col, seqs[i])
                planted.append((col, i))
    return planted


def assert_planted(out, planted):
    for col, i in planted:
        assert col in out.col[int(out.off[i]):int(out.off[i + 1])].tolist(), (col, i)


def run_and_check(case, seqs, threshold, limits, min_chunks, flags=0, **cuts_kw):
    set_limits(case.st, *limits)
    try:
        out = stream(case.st, seqs, threshold, flags)
        cuts = expected_cuts(case, seqs, threshold, limits, **cuts_kw)
    finally:
        set_limits(case.st, 0, 0, 0)
    assert len(cuts) >= min_chunks, len(cuts)
    firsts = [f for f, _, _, _ in cuts]
    assert assert_oracle(case, seqs, threshold, out, firsts) >= 10
    assert_equals_batches(case, seqs, threshold, out, firsts)
    return out, cuts


# ------------------------------------------------------------------------------------------------ 1. cuts by positions
QUERIES_1 = random_seqs(np.random.default_rng(101), 300, 100)
LIMITS_1 = (2000, 8000, 64)
CONFIGS_1 = ((1.0, LIMITS_1), (0.45, LIMITS_1), (0.45, (2000, 8000, 0)))


@pytest.fixture(scope="module")
def planted_1(case):
    firsts = sorted({f for thr, lim in CONFIGS_1 for f, _, _, _ in stream_ref.cuts([100] * 300, K, thr, case.n_cols, H, M, chunk_positions=lim[0],
                                                                                  large_chunk_positions=lim[1], chunk_seqs=lim[2])})
    return plant_around(case, QUERIES_1, firsts)


@pytest.mark.parametrize("threshold,limits", CONFIGS_1)
def test_cuts_by_positions(case, planted_1, threshold, limits):
    """300 queries of 100 bp (70 positions) under limits of 2000 / 8000 positions and 64 sequences: at 1.0 eleven chunks of 28 -- every
    workspace used at least twice -- at 0.45 the large limit applies: it would hold 114, so the cap of 64 sequences ends the chunks, and
    with the library's own cap they are chunks of 114."""
    per_chunk = 28 if threshold == 1.0 else 64 if limits[2] else 114
    out, cuts = run_and_check(case, QUERIES_1, threshold, limits, -(-300 // per_chunk))
    assert [n for _, _, n, _ in cuts[:-1]] == [per_chunk] * (len(cuts) - 1) and not any(b for _, b, _, _ in cuts)
    assert_planted(out, planted_1)
    assert int(out.off[-1]) >= len(planted_1)


def test_cuts_by_positions_every_sample_a_hit(case):
    """threshold 0.0: every sample is a hit of every query, lists beyond what the export kernel carries along, across eleven chunks"""
    seqs = QUERIES_1[:120]
    out, cuts = run_and_check(case, seqs, 0.0, (2000, 700, 64), 9)          # (thresholded: the large limit, set to 700 here: chunks of 10)
    assert np.array_equal(np.diff(out.off.astype(np.int64)), np.full(len(seqs), case.n_cols))
    assert np.array_equal(out.col.reshape(len(seqs), case.n_cols), np.tile(np.arange(case.n_cols, dtype=np.uint32), (len(seqs), 1)))


def test_library_limits_are_back_after_zero(case):
    """0 keeps the library's own value: the same input is one chunk again, and more than 4096 sequences per chunk are refused"""
    from bigsi_amd import _lib
    out = stream(case.st, QUERIES_1, 1.0)
    assert last_chunks(case.st) == [(0, False)]
    assert _lib.lib().bigsi_hip_stream_set_limits(case.st.handle, 0, 0, 4097) == _lib.ERR_INVALID
    set_limits(case.st, 0, 0, 4096)
    assert_same(out, stream(case.st, QUERIES_1, 1.0))
    assert last_chunks(case.st) == [(0, False)]
    set_limits(case.st, 0, 0, 0)
    empty = stream(case.st, [], 1.0, cap=0)
    assert empty.rc == _lib.OK and last_chunks(case.st) == [] and empty.off.tolist() == [0]
    # a call refused before its first chunk reports none either: excluded colours without a limit, k = 0
    stream(case.st, QUERIES_1[:5], 1.0)
    assert last_chunks(case.st) == [(0, False)]
    blob, soff = _lib.pack_seqs(QUERIES_1[:5])
    off, ex = np.zeros(6, np.uint64), np.array([3], np.uint32)
    rc = _lib.lib().bigsi_hip_search_stream_ranked(case.st.handle, blob, _lib.ptr(soff), 5, K, 1.0, 0, None, None, None, _lib.ptr(off), None, None, 0, 0, _lib.ptr(ex), 1)
    assert rc == _lib.ERR_INVALID and last_chunks(case.st) == []
    stream(case.st, QUERIES_1[:5], 1.0)
    rc = _lib.lib().bigsi_hip_search_stream(case.st.handle, blob, _lib.ptr(soff), 5, 0, 1.0, 0, None, None, None, _lib.ptr(off), None, None, 0)
    assert rc == _lib.ERR_INVALID and last_chunks(case.st) == []


# ------------------------------------------------------------------------------------------------ 2. cuts by the sequence cap
READS_2 = random_seqs(np.random.default_rng(102), 300, 40)
LIMITS_2 = (2000, 8000, 16)


@pytest.fixture(scope="module")
def planted_2(case):
    return plant_around(case, READS_2, list(range(0, 300, 16)), base=11)


@pytest.mark.parametrize("threshold", [1.0, 0.6])
def test_cuts_by_the_sequence_cap(case, planted_2, threshold):
    """300 reads of 40 bp (10 positions: the one-launch read kernel) under a cap of 16 sequences: nineteen chunks of 16 whatever the
    position limit.  At 0.6 six of ten k-mers make a hit: a few random columns per read beside the planted ones."""
    out, cuts = run_and_check(case, READS_2, threshold, LIMITS_2, 19)
    assert [f for f, _, _, _ in cuts] == list(range(0, 300, 16))
    assert_planted(out, planted_2)


# ------------------------------------------------------------------------------------------------ 2b. the rounding to whole launches
def rounding_shape(n_cols):
    """(sequences per chunk, queries per row-AND launch): a cap between two and three launches on either index (2500 of 1024; the
    library's own 4096 of 1792)"""
    launch_q = stream_ref.exact_launch_queries(-(-n_cols // 64))
    assert launch_q == (1024 if n_cols == WIDE else 1792)
    return min(2 * launch_q + launch_q // 2 - 60, stream_ref.CHUNK_SEQS), launch_q


@pytest.fixture(scope="module")
def reads_2b(case):
    cap, launch_q = rounding_shape(case.n_cols)
    rng = np.random.default_rng(112)
    letters = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(2 * cap, 40))]
    seqs = [row.tobytes().decode("ascii") for row in letters]
    for col, i in ((case.n_cols - 1, 2 * launch_q - 1), (6, 2 * launch_q), (70, cap - 1), (71, cap), (200, 4 * launch_q - 1), (201, 4 * launch_q)):
        case.plant(col, seqs[i])          # either side of the rounded cuts, and of where the cap alone would have cut
    return seqs


@pytest.mark.parametrize("kind", ["remainder", "large last chunk", "thresholded", "forced band"])
def test_exact_chunks_end_on_whole_launches(case, reads_2b, kind):
    """The second half of the cut rule, seen on the device: reads of 40 bp (10 positions, lists far under 1024 rows: no band sweep
    unforced) under a cap of 2.5 launches' worth of sequences.  An exact chunk with chunks behind it ends on two whole launches; the
    last chunk keeps its size, also when it holds more than two launches; a thresholded chunk and a band chunk are not rounded."""
    from bigsi_amd import _lib
    cap, launch_q = rounding_shape(case.n_cols)
    n, thr, flags, want = {"remainder": (2 * cap, 1.0, 0, [(0, 2 * launch_q), (2 * launch_q, 2 * launch_q), (4 * launch_q, 2 * cap - 4 * launch_q)]),
                           "large last chunk": (2 * launch_q + cap - 7, 1.0, 0, [(0, 2 * launch_q), (2 * launch_q, cap - 7)]),
                           "thresholded": (2 * cap, 0.6, 0, [(0, cap), (cap, cap)]),
                           "forced band": (2 * cap, 1.0, _lib.RUN_BAND_SWEEP, [(0, cap), (cap, cap)])}[kind]
    assert cap - 7 >= 2 * launch_q
    seqs, limits = reads_2b[:n], (1 << 20, 1 << 22, cap)
    set_limits(case.st, *limits)
    try:
        out = stream(case.st, seqs, thr, flags)
        cuts = expected_cuts(case, seqs, thr, limits, flags_band_sweep=bool(flags))
    finally:
        set_limits(case.st, 0, 0, 0)
    assert [(f, c) for f, _, c, _ in cuts] == want and [b for _, b, _, _ in cuts] == [bool(flags)] * len(cuts)
    firsts = [f for f, _, _, _ in cuts]
    assert assert_oracle(case, seqs, thr, out, firsts + [cap, 2 * launch_q, 4 * launch_q]) >= n // 7
    assert_equals_batches(case, seqs, thr, out, firsts)
    if thr == 1.0:
        assert 6 in out.col[int(out.off[2 * launch_q]):int(out.off[2 * launch_q + 1])].tolist()


# ------------------------------------------------------------------------------------------------ 3. shapes changing under one workspace
def mixed_input():
    rng = np.random.default_rng(103)
    reads, longs = random_seqs(rng, 20, 40), random_seqs(rng, 3, 5000)
    nothing = [rand_seq(rng, K - 2), "", rand_seq(rng, K - 1), "ACGT"]
    return reads + longs + nothing + random_seqs(rng, 30, 40)


MIXED_3 = mixed_input()


@pytest.fixture(scope="module")
def planted_3(case):
    planted = []
    for col, i in ((case.n_cols - 1, 19), (5, 20), (130, 22), (64, 27), (200, 12), (63, 56)):
        case.plant(col, MIXED_3[i])
        planted.append((col, i))
    return planted


@pytest.mark.parametrize("threshold", [1.0, 0.5])
@pytest.mark.parametrize("chunk_seqs", [2, 4])
def test_shapes_changing_under_one_workspace(case, planted_3, threshold, chunk_seqs):
    """20 reads, three queries of 5000 bp (each alone over the limit of 2000 positions; 4970 positions: K1's global route), four sequences
    without a k-mer, 30 reads.  With two sequences per chunk, chunks 6, 10, 14 and 18 -- one workspace -- are reads (the read kernel),
    a long query, the two last sequences without a k-mer (nothing to search) and reads again; with four per chunk the four without a
    k-mer are one chunk.  Every query against the oracle.  Then the same index, the input reversed: the workspaces outlive the call."""
    limits = (2000, 2000, chunk_seqs)
    set_limits(case.st, *limits)
    try:
        out = stream(case.st, MIXED_3, threshold)
        cuts = expected_cuts(case, MIXED_3, threshold, limits)
        back = MIXED_3[::-1]
        rev = stream(case.st, back, threshold)
        rev_cuts = expected_cuts(case, back, threshold, limits)
    finally:
        set_limits(case.st, 0, 0, 0)
    shape = [(f, n) for f, _, n, _ in cuts]
    if chunk_seqs == 2:
        assert shape[6] == (12, 2) and shape[10] == (20, 1) and shape[14] == (25, 2) and shape[18] == (33, 2) and len(shape) >= 27
    else:
        assert shape[5:9] == [(20, 1), (21, 1), (22, 1), (23, 4)] and len(shape) >= 15
    everything = range(len(MIXED_3))
    assert assert_oracle(case, MIXED_3, threshold, out, [], everything) == len(MIXED_3) - 4
    assert_planted(out, planted_3)
    assert len(rev_cuts) >= 15 and assert_oracle(case, back, threshold, rev, [], everything) == len(MIXED_3) - 4
    # reversed input, reversed lists
    n = len(MIXED_3)
    assert np.array_equal(rev.nu, out.nu[::-1]) and np.array_equal(rev.mk, out.mk[::-1])
    for i in everything:
        a, b = slice(int(out.off[i]), int(out.off[i + 1])), slice(int(rev.off[n - 1 - i]), int(rev.off[n - i]))
        assert np.array_equal(out.col[a], rev.col[b]) and np.array_equal(out.cnt[a], rev.cnt[b]), i
    assert_equals_batches(case, MIXED_3, threshold, out, [f for f, _ in shape])


# ------------------------------------------------------------------------------------------------ 4. edges of the rule on the device
def test_edges_of_the_rule(case):
    from bigsi_amd import _lib
    rng = np.random.default_rng(104)
    limit = 500
    limits = (limit, limit, 64)
    set_limits(case.st, *limits)
    try:
        # one sequence
        one = [rand_seq(rng, 100)]
        out = stream(case.st, one, 1.0)
        assert expected_cuts(case, one, 1.0, limits) == [(0, False, 1, 70)]
        assert_oracle(case, one, 1.0, out, [0])
        # a sequence of exactly the limit stays in its chunk, one of limit + 1 starts the next; a last chunk of exactly one sequence
        for thr in (1.0, 0.5):
            for extra, want in ((0, [(0, 3), (3, 7), (10, 1)]), (1, [(0, 2), (2, 2), (4, 7), (11, 1)])):
                seqs = [rand_seq(rng, 100), rand_seq(rng, 100), rand_seq(rng, limit - 140 + extra + K - 1)] + random_seqs(rng, 7 + extra, 100) + [rand_seq(rng, 100)]
                case.plant(17 + extra, seqs[2])
                case.plant(case.n_cols - 1, seqs[-1])
                out = stream(case.st, seqs, thr)
                cuts = expected_cuts(case, seqs, thr, limits)
                assert [(f, n) for f, _, n, _ in cuts] == want
                assert assert_oracle(case, seqs, thr, out, [], range(len(seqs))) == len(seqs)
                assert_planted(out, [(17 + extra, 2), (case.n_cols - 1, len(seqs) - 1)])
        # decreasing offsets in the third chunk: refused, the chunks launched until then are the first two
        seqs = random_seqs(rng, 40, 100)          # chunks of 7
        case.plant(9, seqs[15])
        blob, soff = _lib.pack_seqs(seqs)
        bad = soff.copy()
        bad[17] = bad[16] - 1
        res = stream(case.st, None, 1.0, cap=64, packed=(blob, bad))
        assert res.rc == _lib.ERR_INVALID and b"non-decreasing" in _lib.lib().bigsi_hip_last_error()
        assert last_chunks(case.st) == [(0, False), (7, False)]
        # ... and a good call behind it is right: the workspaces were dropped
        out = stream(case.st, seqs, 1.0)
        cuts = expected_cuts(case, seqs, 1.0, limits)
        assert [f for f, _, _, _ in cuts] == [0, 7, 14, 21, 28, 35]
        assert assert_oracle(case, seqs, 1.0, out, [], range(len(seqs))) == len(seqs)
        assert_planted(out, [(9, 15)])
    finally:
        set_limits(case.st, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ 5. hit capacity running out in the middle
@pytest.mark.parametrize("kind", ["positions", "reads", "every sample"])
def test_hit_capacity_runs_out_in_a_middle_chunk(case, planted_1, planted_2, kind):
    from bigsi_amd import _lib
    seqs, thr, limits = {"positions": (QUERIES_1, 1.0, LIMITS_1), "reads": (READS_2, 0.6, LIMITS_2), "every sample": (QUERIES_1[:90], 0.0, (2000, 700, 64))}[kind]
    set_limits(case.st, *limits)
    try:
        full = stream(case.st, seqs, thr)                    # (sizing call with capacity 0 and NULL lists, then exactly off[-1]: same offsets)
        cuts = expected_cuts(case, seqs, thr, limits)
        firsts = [f for f, _, _, _ in cuts] + [len(seqs)]
        assert len(cuts) >= 6
        lo, hi = int(full.off[firsts[2]]), int(full.off[firsts[3]])
        assert hi - lo >= 2, "the third chunk needs hits for the capacity to end inside it"
        cap = lo + (hi - lo) // 2
        short = stream(case.st, seqs, thr, cap=cap)
        assert short.rc == _lib.ERR_CAPACITY and last_chunks(case.st) == [(f, b) for f, b, _, _ in cuts]
        assert np.array_equal(short.off, full.off) and np.array_equal(short.nk, full.nk) and np.array_equal(short.nu, full.nu) and np.array_equal(short.mk, full.mk)
        assert np.array_equal(short.col[:lo], full.col[:lo]) and np.array_equal(short.cnt[:lo], full.cnt[:lo])
        again = stream(case.st, seqs, thr, cap=int(short.off[-1]))
        assert again.rc == _lib.OK
        assert_same(again, full)
        # one entry short of enough: the last chunk overflows
        short = stream(case.st, seqs, thr, cap=int(full.off[-1]) - 1)
        lo = int(full.off[firsts[-2]])
        assert short.rc == _lib.ERR_CAPACITY and np.array_equal(short.off, full.off) and np.array_equal(short.col[:lo], full.col[:lo])
    finally:
        set_limits(case.st, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ 6. scored stream across cuts
def scored_input(case):
    rng = np.random.default_rng(106)
    seqs = random_seqs(rng, 150, 100) + [rand_seq(rng, 31 + 64), rand_seq(rng, 31 + 63), rand_seq(rng, 300)]
    seqs[39] = seqs[39][:50] * 2                         # repeated k-mers
    for j, i in enumerate(range(0, len(seqs), 3)):       # whole, a prefix and a suffix: exact hits and hits with gaps to score
        case.plant((7 + 31 * j) % case.n_cols, seqs[i])
        case.plant((8 + 31 * j) % case.n_cols, seqs[i][:70])
        case.plant((case.n_cols - 1 - 29 * j) % case.n_cols, seqs[i][25:])
    for c, i in ((4001 % case.n_cols, 150), (4002 % case.n_cols, 151), (4003 % case.n_cols, 152)):          # 65, 64 and 270 positions: two words, exactly one, five
        case.plant(c, seqs[i])
    return seqs


def assert_scored_against_references(case, seqs, threshold, s, indices):
    from bigsi_amd.scoring import SCORE_KEYS, Scorer, score_columns, unpack_presence
    from presence_reference import presence_strings
    total = int(s.off[-1])
    assert int(s.boff[total]) == s.need == s.bits.size
    text, cols, scalar = unpack_presence(s.bits, s.boff[:total + 1]), score_columns(s.rec[:total], case.n_cols), Scorer(case.n_cols)
    hits = 0
    for i in indices:
        lo, hi = int(s.off[i]), int(s.off[i + 1])
        want = presence_strings(case.orc, seqs[i], s.col[lo:hi])
        for t, w in zip(range(lo, hi), want):
            assert text[8 * int(s.boff[t]):8 * int(s.boff[t]) + int(s.nk[i])] == w, (i, t)
            assert int(s.boff[t + 1] - s.boff[t]) == (int(s.nk[i]) + 63) // 64 * 8
            assert {key: c[t] for key, c in zip(SCORE_KEYS, cols)} == scalar.score(w), (i, t)
            assert s.rec["percent_kmers_found"][t] == round(100 * float(s.cnt[t]) / int(s.nu[i]), 2) and s.rec["num_kmers"][t] == s.nk[i]
            hits += 1
    return hits


@pytest.mark.parametrize("threshold", [1.0, 0.45])
def test_scored_stream_across_cuts(case, threshold):
    from bigsi_amd import _lib
    if not hasattr(case, "scored_seqs"):
        case.scored_seqs = scored_input(case)
    seqs = case.scored_seqs
    limits = (2000, 8000, 64)                            # (a scored stream takes the small limit at any threshold)
    plain = stream(case.st, seqs, threshold)
    total = int(plain.off[-1])
    assert total >= 50
    whole = stream_scored(case.st, seqs, threshold, total, 1 << 22)          # the library's limits: one chunk
    assert whole.rc == _lib.OK and last_chunks(case.st) == [(0, False)]
    set_limits(case.st, *limits)
    try:
        s = stream_scored(case.st, seqs, threshold, total, whole.need)
        assert s.rc == _lib.OK
        cuts = expected_cuts(case, seqs, threshold, limits, scored=True)
        firsts = [f for f, _, _, _ in cuts] + [len(seqs)]
        assert len(cuts) >= 6 and not any(b for _, b, _, _ in cuts)
        # hit lists: the plain stream's; bits, offsets and records: the uncut run's, whole, and the references' around the cuts
        assert_same(s, plain)
        assert s.need == whole.need and np.array_equal(s.boff, whole.boff) and np.array_equal(s.bits, whole.bits[:whole.need]) and np.array_equal(s.rec, whole.rec)
        assert_oracle(case, seqs, threshold, s, firsts[:-1])
        assert assert_scored_against_references(case, seqs, threshold, s, range(len(seqs))) == total
        # the bit buffer ends in the third chunk: CAPACITY, bits_needed the full run's, lists and offsets complete, the bits of the
        # chunks before it in place, nothing behind the capacity (stream_scored checks the guard bytes)
        b_lo, b_hi = int(s.boff[int(s.off[firsts[2]])]), int(s.boff[int(s.off[firsts[3]])])
        assert b_hi - b_lo >= 16
        bcap = b_lo + (b_hi - b_lo) // 2 // 8 * 8
        short = stream_scored(case.st, seqs, threshold, total, bcap)
        assert short.rc == _lib.ERR_CAPACITY and short.need == s.need and last_chunks(case.st) == [(f, b) for f, b, _, _ in cuts]
        assert_same(short, plain)
        assert np.array_equal(short.boff, s.boff) and np.array_equal(short.bits[:b_lo], s.bits[:b_lo])
        n_lo = int(s.off[firsts[2]])
        assert np.array_equal(short.rec[:n_lo], s.rec[:n_lo])
        # the hit buffer ends in the third chunk: bits_needed -- from here on the host's estimate from sequence lengths -- still the
        # full run's
        h_lo, h_hi = int(s.off[firsts[2]]), int(s.off[firsts[3]])
        assert h_hi - h_lo >= 2
        short = stream_scored(case.st, seqs, threshold, h_lo + (h_hi - h_lo) // 2, whole.need)
        assert short.rc == _lib.ERR_CAPACITY and short.need == s.need and np.array_equal(short.off, s.off)
        assert np.array_equal(short.col[:h_lo], s.col[:h_lo]) and np.array_equal(short.boff[:h_lo + 1], s.boff[:h_lo + 1])
        assert np.array_equal(short.bits[:int(s.boff[h_lo])], s.bits[:int(s.boff[h_lo])]) and np.array_equal(short.rec[:h_lo], s.rec[:h_lo])
        # ... and with no room at all (the sizing call)
        short = stream_scored(case.st, seqs, threshold, 0, 0)
        assert short.rc == _lib.ERR_CAPACITY and short.need == s.need and np.array_equal(short.off, s.off)
        # the retry with what was reported
        again = stream_scored(case.st, seqs, threshold, int(short.off[-1]), short.need)
        assert again.rc == _lib.OK and np.array_equal(again.bits, s.bits) and np.array_equal(again.rec, s.rec) and np.array_equal(again.boff, s.boff)
    finally:
        set_limits(case.st, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ 7. ranked stream across cuts
def topn(colours, counts, n, exact):
    """The reference's order (ascending colour; thresholded: stable sort by count, descending) cut to n, back in ascending colour."""
    colours, counts = np.asarray(colours), np.asarray(counts)
    order = np.arange(colours.size) if exact else np.lexsort((colours, -counts.astype(np.int64)))
    keep = np.sort(order[:n])
    return colours[keep], counts[keep]


def ranked_input(case):
    rng = np.random.default_rng(107)
    seqs = random_seqs(rng, 260, 100) + random_seqs(rng, 40, 40)
    for j, i in enumerate(range(0, len(seqs), 2)):
        s = seqs[i]
        for c, piece in ((3 + 13 * j, s), (4 + 13 * j, s), (5 + 13 * j, s[: len(s) * 3 // 4]), (case.n_cols - 1 - 7 * j, s[len(s) // 5:]), (700 + j, s), (1200 + j, s), (2000 + j, s)):
            case.plant(c % case.n_cols, piece)
    return seqs


@pytest.mark.parametrize("threshold", [1.0, 0.45])
def test_ranked_stream_across_cuts(case, threshold):
    """limit 1 and 3 with an excluded set that holds planted columns, across cuts by positions: every list is the full list (oracle-checked)
    put through the ranking rule -- excluded colours out, the highest counts, ties to the lowest colours, ascending colour."""
    if not hasattr(case, "ranked_seqs"):
        case.ranked_seqs = ranked_input(case)
    seqs = case.ranked_seqs
    limits = (2000, 4000, 64)
    excluded = np.array(sorted({3, 4, 700 % case.n_cols, 701 % case.n_cols, 16, 5 + 13 * 7, case.n_cols - 1}), np.uint32)
    set_limits(case.st, *limits)
    try:
        full = stream(case.st, seqs, threshold)
        cuts = expected_cuts(case, seqs, threshold, limits)
        firsts = [f for f, _, _, _ in cuts]
        assert len(cuts) >= 5
        assert_oracle(case, seqs, threshold, full, firsts)
        assert int(np.diff(full.off.astype(np.int64)).max()) >= 5          # (five whole plants per second query)
        for limit in (1, 3):
            got = stream(case.st, seqs, threshold, limit=limit, excluded=excluded)
            assert last_chunks(case.st) == [(f, b) for f, b, _, _ in cuts]
            assert np.array_equal(got.nk, full.nk) and np.array_equal(got.nu, full.nu) and np.array_equal(got.mk, full.mk)
            cut_short = 0
            for i in range(len(seqs)):
                c, n = full.col[int(full.off[i]):int(full.off[i + 1])], full.cnt[int(full.off[i]):int(full.off[i + 1])]
                keep = ~np.isin(c, excluded)
                wc, wn = topn(c[keep], n[keep], limit, threshold == 1.0)
                lo, hi = int(got.off[i]), int(got.off[i + 1])
                assert np.array_equal(got.col[lo:hi], wc) and np.array_equal(got.cnt[lo:hi], wn), (limit, i)
                cut_short += int(keep.sum()) > limit
            assert cut_short >= 100
            assert_equals_batches(case, seqs, threshold, got, firsts, limit=limit, excluded=excluded)
        # the workspaces outlive the call and every call sets its own limit: off again
        assert_same(stream(case.st, seqs, threshold), full)
    finally:
        set_limits(case.st, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ 8. band sweep in a stream
def and_launches(st):
    from bigsi_amd import _lib
    s = _lib.Stats()
    _lib.check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(s), 0))
    return int(s.and_launches_total)


def band_set_limits(st, windows, segs):
    from bigsi_amd import _lib
    _lib.check(_lib.lib().bigsi_hip_band_set_limits(st.handle, windows, segs))


@pytest.mark.parametrize("windows,segs", [(3, 1), (3, 2), (2000, 1), (2000, 2)])
def test_forced_band_sweep_in_a_stream(case, planted_1, windows, segs):
    """BIGSI_RUN_BAND_SWEEP in the stream's flags, a large limit of 2000 positions: eleven band chunks of 28 queries share the four
    workspaces, each chunk's launches are the band plan's (groups of segments x windows), results unchanged."""
    from bigsi_amd import _lib
    limits = (1000, 2000, 64)
    wv = -(-case.n_cols // 64)
    plain = stream(case.st, QUERIES_1, 1.0)
    set_limits(case.st, *limits)
    band_set_limits(case.st, windows, segs)
    try:
        before = and_launches(case.st)
        out = stream(case.st, QUERIES_1, 1.0, flags=_lib.RUN_BAND_SWEEP, cap=int(plain.off[-1]))
        grown = and_launches(case.st) - before
        cuts = expected_cuts(case, QUERIES_1, 1.0, limits, flags_band_sweep=True, band_windows=windows, band_segs=segs)
        assert len(cuts) >= 9 and all(b for _, b, _, _ in cuts) and [n for _, _, n, _ in cuts[:-1]] == [28] * (len(cuts) - 1)
        assert grown == sum(stream_ref.band_plan(n, wv, mp, H, M, True, windows, segs)[1] for _, _, n, mp in cuts)
        assert grown == len(cuts) * -(-(-(-wv // 128)) // segs) * windows
        assert out.rc == _lib.OK
        assert_same(out, plain)
        # no band chunk with forced counts or below 1.0, flag or not
        for thr, flags in ((1.0, _lib.RUN_BAND_SWEEP | _lib.RUN_FORCE_COUNTS), (0.45, _lib.RUN_BAND_SWEEP)):
            other = stream(case.st, QUERIES_1, thr, flags=flags)
            chunks = last_chunks(case.st)
            assert len(chunks) >= 3 and not any(b for _, b in chunks)
            assert chunks == [(f, b) for f, b, _, _ in stream_ref.cuts([100] * 300, K, thr, case.n_cols, H, M, flags_force_counts=thr == 1.0, flags_band_sweep=True,
                                                                       chunk_positions=limits[0], large_chunk_positions=limits[1], chunk_seqs=limits[2])]
            if thr == 1.0:
                assert np.array_equal(other.off, plain.off) and np.array_equal(other.col, plain.col)
    finally:
        band_set_limits(case.st, 0, 0)
        set_limits(case.st, 0, 0, 0)
    firsts = [f for f, _, _, _ in cuts]
    assert_oracle(case, QUERIES_1, 1.0, out, firsts)
    assert_planted(out, planted_1)


def test_unforced_band_sweep_and_a_recut_remainder(wide):
    """The planner's own decision inside a stream.  On 1009 rows of 130 words the band sweep takes a chunk from 3072 queries of 342
    positions on (lists of 1026 rows: plan_row_and sorts them from 1024 rows; 100 bp queries are never taken unforced) -- the count comes
    from the restatement of plan_band_sweep.  6500 queries of 372 bp under a large limit of 3072 x 342 positions and a small one of
    300 x 342: two band chunks of 3072, then the remainder of 356 -- too few for the route -- cut again at the small limit into a
    chunk of 300 and one of 56: band and non-band chunks in one call, a band chunk in a workspace first, a recut one behind it."""
    from bigsi_amd import _lib
    case = wide
    wv, length = -(-case.n_cols // 64), 372
    pos = length - K + 1
    n_band = next(n for n in range(1, 9000) if stream_ref.band_plan(n, wv, pos, H, M)[0])
    assert n_band == 3072 and not stream_ref.band_plan(n_band, wv, pos - 1, H, M)[0] and not stream_ref.band_plan(4096, wv, 70, H, M)[0]
    rng = np.random.default_rng(108)
    letters = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(6500, length))]
    seqs = [row.tobytes().decode("ascii") for row in letters]
    limits = (300 * pos, n_band * pos, 4096)
    want = stream_ref.cuts([length] * len(seqs), K, 1.0, case.n_cols, H, M, chunk_positions=limits[0], large_chunk_positions=limits[1], chunk_seqs=limits[2])
    assert [(f, b, n) for f, b, n, _ in want] == [(0, True, 3072), (3072, True, 3072), (6144, False, 300), (6444, False, 56)]
    firsts = [f for f, _, _, _ in want]
    planted = plant_around(case, seqs, firsts, base=21)
    set_limits(case.st, *limits)
    try:
        before = and_launches(case.st)
        out = stream(case.st, seqs, 1.0, cap=4096)
        grown = and_launches(case.st) - before
        assert out.rc == _lib.OK
        cuts = expected_cuts(case, seqs, 1.0, limits)
        assert cuts == want
        # the band chunks' launches are the band plan's: one launch of both segments each (the second segment's two words ride along)
        assert stream_ref.band_plan(3072, wv, pos, H, M) == (True, 1) and grown == 2 + 2
        # with forced counts or below 1.0 no chunk is band
        for thr, flags in ((1.0, _lib.RUN_FORCE_COUNTS), (0.45, 0)):
            other = stream(case.st, seqs[:3300], thr, flags=flags)
            chunks = last_chunks(case.st)
            assert not any(b for _, b in chunks)
            if thr == 1.0:
                assert np.array_equal(other.off, out.off[:3301]) and np.array_equal(other.col, out.col[:int(out.off[3300])])
            assert chunks == [(f, b) for f, b, _, _ in stream_ref.cuts([length] * 3300, K, thr, case.n_cols, H, M, flags_force_counts=thr == 1.0,
                                                                       chunk_positions=limits[0], large_chunk_positions=limits[1], chunk_seqs=limits[2])]
    finally:
        set_limits(case.st, 0, 0, 0)
    total = int(out.off[-1])
    out = Out(out.rc, out.nk, out.nu, out.mk, out.off, out.col[:total], out.cnt[:total])
    assert_planted(out, planted)
    assert_oracle(case, seqs, 1.0, out, firsts)
    # the whole output against default-route batches (1300 queries each: sliced or plain row-AND launches, never the band sweep)
    for lo in range(0, len(seqs), 1300):
        part = seqs[lo:lo + 1300]
        b = case.st.new_batch(part, K)
        before = and_launches(case.st)
        b.run(1.0, sparse_counts=True)
        assert not stream_ref.band_plan(len(part), wv, pos, H, M)[0] and and_launches(case.st) - before >= 1
        bnk, bnu, bmk = b.unique()
        boff, bcol, bcnt = b.hits()
        b.close()
        hi = lo + len(part)
        assert np.array_equal(out.nk[lo:hi], bnk) and np.array_equal(out.nu[lo:hi], bnu) and np.array_equal(out.mk[lo:hi], bmk)
        assert np.array_equal(out.off[lo:hi + 1].astype(np.int64) - int(out.off[lo]), boff.astype(np.int64))
        assert np.array_equal(out.col[int(out.off[lo]):int(out.off[hi])], bcol) and np.array_equal(out.cnt[int(out.off[lo]):int(out.off[hi])], bcnt)
