"""The "knock-out" index of the exact-search tests (a plain module: nothing here is collected): for ONE main query an index in which
every column but a handful holds every row of the query EXCEPT ONE, built on the host from numpy and oracle.coracle alone, with its
numpy reference, and the table of cases (CASES) that tests/test_knockout_host.py pins on the CPU and tests/test_gpu_knockout.py runs
on the device.

Why.  On random noise plus planted columns a kernel that SKIPS a row is invisible: noise is zero after a dozen rows anyway and a
planted column survives any omission.  Here a skipped row turns the column that knocks it out into a hit.

Method.  k = 31.  R is the ascending array of the DISTINCT row ids of the main query's unique k-mers, r = len(R).  `order` is a
permutation of range(r) whose head holds the telling list positions of the case (named_positions: first and last entry of the
hash-order and of the address-order list, both neighbours of every slice cut i x per and of every unroll tail, every window bound of
a band sweep), the rest seeded.  A column is FULL (every row of R set) or the KNOCK-OUT of one row R[j] (every row of R set except
R[j]).  The named edge columns of every 1 KiB segment (count_staircase.edge_columns: both ends of its first two words, its last
column, both sides of every 128-word tile and segment cut) are FULL; the i-th of the OTHER columns of segment s = c // 8192 knocks
out order[i % r] (counting the other columns only, so that an edge column takes nobody's knock-out away).  Only the rows of R are
written; every other row of the index stays zero.  A segment with at least r such columns knocks every row of R; a narrower (ragged
last) segment covers the head of `order`, which is why the telling positions stand there.  Duplicate row ids -- two k-mers that
collide on a row -- are knocked once: skipping one of two equal references is legitimate.

Fillers are substrings of the main query (count_staircase.make_fillers' rule): their rows F are a subset of R, column c is a hit of
the filler iff its knocked row is not in F, and a skipped row of a filler shows in the column that knocks it.  Among them one
sequence shorter than k, one of exactly k and one equal to the main query; in batches of more than a thousand queries, and on wide
indexes, they are long (`fmin` of the main's positions at least) so that the hit lists stay small.

reference(seq) is Staircase.reference itself: generic, it does not trust the construction -- per column the number of unique k-mers
all of whose h WRITTEN rows have the bit.  An exact hit is count == u (none when u == 0), a thresholded hit count >= ceil(u x thr)
in double.  counts_of_batch computes the same for a whole batch as one matrix product over the batch's distinct k-mers; the host test
holds it against reference().
"""
import numpy as np

from count_staircase import K, Staircase, edge_columns, make_main, min_kmers, threshold_for   # noqa: F401  (re-exported)
from oracle import coracle

SEG_COLS, SEG_WORDS = 8192, 128
M = 20011
BIG_M = 5400001                      # > 4700 queries x 286 positions x 4 rows
K1_WAVE, K1_LDS, K1_GLOBAL = 1, 2, 3
NONE, BY_K1, SORT256, SORT1024 = 0, 1, 2, 3
SORT_BUCKETS = 8192


# --------------------------------------------------------------------------------------------- the launch rule's small parts, restated
def sort_shift(m, buckets):
    s = 0
    while m and ((m - 1) >> s) >= buckets:
        s += 1
    return s


def band_window(m, w, W, shift):
    nb = ((m - 1) >> shift) + 1 if m else 0
    return min((nb * w // W) << shift, m), min((nb * (w + 1) // W) << shift, m)


def k1_table_slots(positions, tab_mult):
    t = 2
    while t < tab_mult * positions:
        t <<= 1
    return t


# --------------------------------------------------------------------------------------------- fillers
def filler_positions(n, main_pos, fmax, fmin):
    """k-mer positions of n fillers: the main query again, a sequence shorter than k (-1), exactly k, then short ones (fmin == 0) or
    a walk over [fmin, main_pos]"""
    head = [main_pos, -1, 1]
    if fmin == 0:
        head += [9, 95, 3, 40, 62, 8, 21]
    out = [min(p, fmax) if p > 0 else p for p in head[:n]]
    if fmin:
        span = main_pos - fmin + 1
        out += [fmin + (i * 37) % span for i in range(len(out), n)]
    else:
        step = 37 if fmax % 37 else 41
        out += [1 + (i * step) % fmax for i in range(len(out), n)]
    return out


def make_fillers(main, n, fmax, fmin, seed):
    rng = np.random.default_rng(seed + 1)
    main_pos = len(main) - K + 1
    out = []
    for p in filler_positions(n, main_pos, fmax, fmin):
        length = 20 if p < 0 else p + K - 1
        a = int(rng.integers(0, len(main) - length + 1))
        out.append(main[a:a + length])
    return out


# --------------------------------------------------------------------------------------------- the index
class Knockout(object):
    """The knock-out index of one main sequence.  Attributes: u, krows (uint64[u, h], hash order), hash_list (krows.ravel(): the list
    K1 writes), addr_list (the same, sorted), R, r, order, named (list of (what, index into R)), knocked (int64[n_cols]: the index
    into R a column knocks out, -1 for a FULL column), covered (bool[segments]: the segment knocks every row), row_ids (= R) and
    packed (uint8[r, ceil(n_cols / 8)]): the rows to write."""

    reference = Staircase.reference           # (u, counts int64[n_cols]) of any sequence against the rows written

    def __init__(self, main, h, m, n_cols, seed, slices=(), windows=(), tenth_segment=None):
        self.main, self.h, self.m, self.n_cols, self.seed = main, h, m, n_cols, seed
        first, _ = coracle.unique_kmers(main, K)
        self.u = len(first)
        self.krows = coracle.seq_rows(main, K, h, m)[first].astype(np.uint64)
        self.hash_list = self.krows.ravel()
        self.addr_list = np.sort(self.hash_list, kind="stable")
        self.R = self.row_ids = np.unique(self.hash_list)
        self.r = r = int(self.R.size)
        self.slices, self.windows = tuple(slices), tuple(windows)
        self.named = self.named_positions()
        head = []
        for _, j in self.named:
            if j not in head:
                head.append(j)
        rng = np.random.default_rng(seed)
        rest = rng.permutation(np.setdiff1d(np.arange(r), head))
        self.order = np.concatenate([np.array(head, np.int64), rest.astype(np.int64)])
        assert np.array_equal(np.sort(self.order), np.arange(r))
        self.n_head = len(head)

        self.knocked = np.full(n_cols, -1, np.int64)
        n_segs = -(-n_cols // SEG_COLS)
        self.covered = np.zeros(n_segs, bool)
        self.seg_cover = np.zeros(n_segs, np.int64)         # entries of `order` (from its head) a segment knocks
        wv = -(-n_cols // 64)
        edges = set(edge_columns(n_cols, [SEG_WORDS * i for i in range(1, -(-wv // SEG_WORDS))]))
        for s in range(n_segs):
            lo, hi = s * SEG_COLS, min((s + 1) * SEG_COLS, n_cols)
            cols = np.arange(lo, hi)
            if s == tenth_segment:
                # every column of this segment knocks a row of the first tenth of the address-ordered list and none is FULL: the
                # running AND of the whole wavefront is zero after that tenth (what BIGSI_RUN_EARLY_EXIT looks for)
                pool = self.order[self.order < max(r // 10, 1)]
            else:
                cols = np.array([c for c in cols if c not in edges and c not in (lo, lo + 63, lo + 64, lo + 127, hi - 1)], np.int64)
                pool = self.order
            self.knocked[cols] = pool[np.arange(cols.size) % pool.size]
            self.seg_cover[s] = min(cols.size, pool.size) if s != tenth_segment else 0
            self.covered[s] = s != tenth_segment and cols.size >= r
        bits = np.ones((r, n_cols), np.uint8)
        kc = np.flatnonzero(self.knocked >= 0)
        bits[self.knocked[kc], kc] = 0
        self.packed = np.packbits(bits, axis=1)
        self.bits = bits.view(np.bool_)
        self.bits.setflags(write=False)

    # ---- the telling positions
    def named_positions(self):
        """(what, index into R) of the list positions where a kernel can lose a row"""
        Rall = int(self.hash_list.size)
        out = []

        def add(what, lst, p):
            if 0 <= p < Rall:
                out.append(("%s[%d] %s" % ("hash" if lst is self.hash_list else "addr", p, what), int(np.searchsorted(self.R, lst[p]))))

        for lst in (self.hash_list, self.addr_list):
            add("first", lst, 0)
            add("last", lst, Rall - 1)
        for lst in (self.addr_list, self.hash_list):
            for W, shift in self.windows:
                if lst is self.addr_list:
                    for w in range(1, min(W, 64)):
                        p = int(np.searchsorted(self.addr_list, band_window(self.m, w, W, shift)[0]))
                        add("before window %d of %d" % (w, W), lst, p - 1)
                        add("first of window %d of %d" % (w, W), lst, p)
            for U in (8, 4, 2):
                add("before the tail of unroll %d" % U, lst, Rall - Rall % U - 1)
                add("first of the tail of unroll %d" % U, lst, Rall - Rall % U)
            for S in self.slices:
                per = -(-Rall // S)
                for i in range(1, S):
                    add("last of slice %d of %d" % (i - 1, S), lst, i * per - 1)
                    add("first of slice %d of %d" % (i, S), lst, i * per)
        return out

    # ---- where a row sits: for a failure's message
    def where(self, j):
        """the positions of R[j] in the hash-order and the address-order list, with their slices and windows"""
        row = self.R[j]
        Rall = int(self.hash_list.size)
        hp, ap = np.flatnonzero(self.hash_list == row).tolist(), np.flatnonzero(self.addr_list == row).tolist()
        s = "row %d: hash-order %s, address-order %s of %d" % (int(row), hp, ap, Rall)
        for S in self.slices:
            per = -(-Rall // S)
            s += "; of %d slices: hash %s, addr %s" % (S, [p // per for p in hp], [p // per for p in ap])
        for W, shift in self.windows:
            s += "; window %d of %d" % (next(w for w in range(W) if band_window(self.m, w, W, shift)[1] > row), W)
        return s

    def explain(self, qi, seq, col):
        j = int(self.knocked[col])
        if j < 0:
            return "query %d, column %d (FULL)" % (qi, col)
        return "query %d (%d positions), column %d knocks %s" % (qi, max(len(seq) - K + 1, 0), col, self.where(j))

    # ---- a whole batch at once
    def counts_of_batch(self, queries, chunk_cols=8192):
        """(u int64[n], counts int32[n, n_cols]): reference() of every query, as one matrix product over the batch's distinct
        k-mers (a k-mer = its h row ids; one with a row that was never written counts nowhere)"""
        n = len(queries)
        us = np.zeros(n, np.int64)
        per_q, keys = [], {}
        for i, q in enumerate(queries):
            first, _ = coracle.unique_kmers(q, K)
            us[i] = len(first)
            ids = []
            if len(first):
                for row in coracle.seq_rows(q, K, self.h, self.m)[first].astype(np.uint64):
                    ids.append(keys.setdefault(row.tobytes(), len(keys)))
            per_q.append(ids)
        kr = np.frombuffer(b"".join(keys.keys()), np.uint64).reshape(len(keys), self.h) if keys else np.zeros((0, self.h), np.uint64)
        idx = np.minimum(np.searchsorted(self.row_ids, kr), self.row_ids.size - 1)
        written = (self.row_ids[idx] == kr).all(axis=1)
        member = np.zeros((n, len(keys)), np.float32)
        for i, ids in enumerate(per_q):
            member[i, ids] = 1.0
        member[:, ~written] = 0.0
        counts = np.zeros((n, self.n_cols), np.int32)
        for c0 in range(0, self.n_cols, chunk_cols):
            held = self.bits[idx[:, 0], c0:c0 + chunk_cols].copy()
            for t in range(1, self.h):
                held &= self.bits[idx[:, t], c0:c0 + chunk_cols]
            counts[:, c0:c0 + chunk_cols] = np.rint(member @ held.astype(np.float32)).astype(np.int32)      # (exact: counts < 2^24)
        return us, counts


# --------------------------------------------------------------------------------------------- the cases
# The smallest shapes that take each route of the exact path.  `route` is what bigsi_hip_batch_last_row_and must report; the host
# test asks the compiled planner (tests/c_host/launch_host.cpp, band_plan_host.cpp) and a case that moves off its route fails there.
# A batch is the main query followed by n_queries - 1 fillers.  kind: "batch" (new_batch / run), "one_call" (search_batch_arrays),
# "reads" (a batch that takes k_reads_fused) or "group" (a device group of two shards on one device).
def _band_route(windows, launches, sorted_by):
    # (of a band run only K1, the sort and the sweep's own launches are pinned: plan_row_and's launches are not taken)
    return dict(slices=None, block=None, tiles=None, n_launches=None, chunk_q=None, last=None, sorted_by=sorted_by, k1_route=K1_LDS,
                preset_by=None, band=(windows, launches), early_exit=0, zero_copy=0)


def _route(slices=1, block=256, tiles=1, n_launches=1, chunk_q=None, last=None, sorted_by=NONE, k1=K1_LDS, preset_by=0, band=None, early=0, zero_copy=0):
    return dict(slices=slices, block=block, tiles=tiles, n_launches=n_launches, chunk_q=chunk_q, last=last or (slices, block, 8),
                sorted_by=sorted_by, k1_route=k1, preset_by=preset_by, band=band, early_exit=early, zero_copy=zero_copy)


def _case(name, n_queries, main_pos, n_cols, route, kind="batch", h=4, m=M, fmax=150, fmin=None, run_kw=None, limits=None, seed=1, **kw):
    if fmin is None:
        fmin = -(-3 * main_pos // 4) if n_queries > 1000 else 0
    return dict(name=name, n_queries=n_queries, main_pos=main_pos, n_cols=n_cols, route=route, kind=kind, h=h, m=m, fmax=min(fmax, main_pos),
                fmin=fmin, run_kw=run_kw or {}, limits=limits, seed=seed, **kw)


_WIDE = dict(n_cols=32832, fmin=258)
CASES = [
    _case("one_sliced", 1, 286, 1200, _route(17, 128, preset_by=1), slices=(17,)),
    _case("few_sliced", 9, 1024, 4400, _route(64, 128, preset_by=1), slices=(64,), fmax=1024),
    _case("one_call", 1, 286, 1200, _route(17, 128, preset_by=1, zero_copy=1), kind="one_call", slices=(17,)),
    _case("plain256_regs", 1024, 286, 1200, _route(sorted_by=BY_K1)),
    _case("plain256_loop", 1024, 1100, 4400, _route(sorted_by=BY_K1)),
    _case("mid64", 1030, 286, 1200, _route(block=64, sorted_by=BY_K1)),
    _case("sort256", 1024, 286, 1200, _route(sorted_by=SORT256, k1=K1_GLOBAL), run_kw=dict(k1_global=True)),
    _case("sort1024", 1024, 600, 2400, _route(sorted_by=SORT1024, k1=K1_GLOBAL), run_kw=dict(k1_global=True)),
    _case("long_global", 1024, 4097, 8200, _route(sorted_by=SORT1024, k1=K1_GLOBAL), h=2, fmax=300, fmin=0),
    _case("hash_order", 1024, 200, 800, _route()),
    # (more than 3072 queries: m is large enough that the batch references a row less than once on average, or the planner would
    # give the batch to the band sweep)
    _case("chunk_sliced_tail", 3700, 286, 1200, _route(n_launches=3, chunk_q=1792, last=(17, 256, 8), sorted_by=BY_K1), slices=(17,), m=BIG_M),
    _case("chunk_mid_tail", 4700, 286, 1200, _route(n_launches=3, chunk_q=1792, last=(1, 64, 8), sorted_by=BY_K1), m=BIG_M),
    _case("wide_tiles64", 205, 286, route=_route(block=64, tiles=5, sorted_by=BY_K1), **_WIDE),
    _case("wide_tiles256", 640, 286, route=_route(tiles=2, last=(1, 256, 4), sorted_by=BY_K1), **_WIDE),
    # k_and_exact<4>: the fewest queries whose rows of 513 words put more than 14.5 MB in flight at 8 loads (464 x 513 x 64 bytes).
    # h = 3 and 285 unique k-mers: 855 rows leave the loop of four a tail of three (at h = 4 every list is whole groups of four); 858
    # row ids per query are fewer than the 1024 from which on the lists are sorted
    _case("unroll4", 464, 287, route=_route(block=64, tiles=5, last=(1, 64, 4)), h=3, **_WIDE),
    _case("early_regs", 1024, 286, 1200, _route(sorted_by=BY_K1, early=1), run_kw=dict(early_exit=True), same_as="plain256_regs"),
    _case("early_sliced", 1, 286, 1200, _route(17, 128, preset_by=1, early=1), run_kw=dict(early_exit=True), slices=(17,), same_as="one_sliced"),
    _case("early_tenth", 1024, 286, 8192 + 1200, _route(sorted_by=BY_K1, early=1), run_kw=dict(early_exit=True), tenth_segment=0),
]
# the band sweep: 301 queries of 70 positions, forced, W windows x S segments per launch; 130 words: the tail segment is one lane
for _W in (1, 3, 16, 2000):
    for _S in (1, 2):
        _groups = 2 if _S == 1 else 1
        CASES.append(_case("band_w%d_s%d" % (_W, _S), 301, 70, 8261,
                           _band_route(_W, _groups * _W, BY_K1 if _W == 1 else SORT256), h=3, m=1009, fmax=70,
                           run_kw=dict(band_sweep=True), limits=(_W, _S), windows=((_W, sort_shift(1009, SORT_BUCKETS)),)))
# m = 100003: the sort's shift is 4 and a bucket holds 16 row ids; 129 words: the tail lane's second word is past the end
CASES.append(_case("band_shift", 301, 70, 8253, _band_route(16, 32, SORT256), h=3, m=100003, fmax=70,
                   run_kw=dict(band_sweep=True), limits=(16, 1), windows=((16, sort_shift(100003, SORT_BUCKETS)),)))
# reads: k_reads_fused (one launch; the planner is not asked) -- a handful of reads (the split workgroup), one word per lane, two
# (slices = 2: the halves of the split workgroup meet at ceil(R / 2), which is where two slices are cut)
CASES += [_case("reads_%s_h%d" % (kind, h), n, 63, n_cols, None, kind="reads", h=h, fmax=63, slices=(2,))
          for kind, n, n_cols in (("split", 40, 200), ("narrow", 300, 200), ("two", 300, 20000)) for h in (2, 3, 4)]
# a device group of two shards (640 + 560 columns) on one device: the shard cut lies inside a knock-out block
CASES.append(_case("group2", 1024, 286, 1200, _route(sorted_by=BY_K1), kind="group", devices=[0, 0]))
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

_built = {}


def build_case(name):
    """(case, knock-out index, queries): built once per process and shared; nobody changes them.  Cases of one geometry share the
    index."""
    if name not in _built:
        c = CASE_BY_NAME[name]
        key = (c["main_pos"], c["h"], c["m"], c["n_cols"], c["seed"], c.get("slices", ()), c.get("windows", ()), c.get("tenth_segment"))
        if key not in _built:
            main = make_main(c["main_pos"], c["seed"])
            _built[key] = Knockout(main, c["h"], c["m"], c["n_cols"], c["seed"], slices=c.get("slices", ()), windows=c.get("windows", ()),
                                   tenth_segment=c.get("tenth_segment"))
        ko = _built[key]
        _built[name] = (c, ko, [ko.main] + make_fillers(ko.main, c["n_queries"] - 1, c["fmax"], c["fmin"], c["seed"]))
    return _built[name]


_refs = {}


def references(name):
    """(u int64[n], counts int32[n, n_cols]) of a case's batch: computed once, shared, never changed"""
    c, ko, queries = build_case(name)
    key = (id(ko), tuple(queries))
    if key not in _refs:
        us, counts = ko.counts_of_batch(queries)
        counts.setflags(write=False)
        _refs[key] = (us, counts)
    return _refs[key]


def planner_input(c, queries):
    """what plan_row_and and k1_plan read of a case's batch: n_seqs, words of a result vector, longest query in positions and bytes"""
    cols = c["n_cols"] if c["kind"] != "group" else -(-(-(-c["n_cols"] // len(c["devices"]))) // 64) * 64
    return dict(n_seqs=len(queries), wv=-(-cols // 64), max_pos=max(max(len(q) - K + 1, 0) for q in queries), max_len=max(len(q) for q in queries))
