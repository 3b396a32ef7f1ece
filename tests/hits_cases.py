"""The chosen hit patterns of the hit-list tests (a plain module: nothing here is collected): indexes whose hit lists are chosen, not
drawn -- empty, every column, the first and the last column alone, the last column of one word with the first of the next at every
thread, chunk and group cut of K4 (k_hits_totals / k_hits_write), totals that sit exactly on the export's size and on the lists'
capacity -- built on the host from numpy and oracle.coracle alone, with their numpy reference and the path every call is built for,
and the table of cases (CASES) that tests/test_hits_cases_host.py pins on the CPU and tests/test_gpu_hit_lists.py runs on the device.

Method.  k = 31.  A query is ONE k-mer position (an exact run: a hit is a column of the k-mer's rows) or TWO (a thresholded run at
0.5: min_kmers = ceil(2 x 0.5) = 1, a hit is a column of either k-mer and its count is 1 or 2).  The rows of a query's k-mers are
written with put_rows as a chosen column pattern -- of a two-k-mer query the first k-mer gets the pattern's columns c with c % 3 != 2,
the second those with c % 3 != 1, so that the count of a hit is 2 when c % 3 == 0 and 1 otherwise: a count read at a wrong column
shows.  Every other row of the index stays zero, and sequences are re-drawn until all row ids of a case are distinct (seq_rows), so
that no query sees another's pattern.  h = 1, which keeps two-position queries off the one-launch read kernel (it exists for
h = 2 .. 4); the read cases take h = 2 and n_cols = 128 and are that kernel's.

reference() is generic: it does not trust the construction.  For every query it takes the rows actually written, ANDs each unique
k-mer's h rows (a row that was never written is zero), counts over the unique k-mers, and lists the columns with count == u (exact;
none when u = 0) or count >= ceil(u x threshold) in double (thresholded; u = 0: every column, count 0) in ascending colour.

A case is an index, its queries and its calls: a call is the list of queries that go to the device together -- through the one-call
search (kinds "one_call" and "reads": bigsi_hip_search_batch, whose workspace, and with it the capacity of the device lists, lives
on from call to call) or through a batch object (kinds "batch" and "group": new_batch / run / hits).  paths() says for every call
which way it goes through K4, the export and collect: what bigsi_hip_hits_last_path must report.  plan_hits and export_spec below
restate the rule of bigsi_amd/csrc/bigsi_launch.hpp; the host test holds them against the compiled header."""
import math

import numpy as np

from oracle import coracle

K = 31
THRESHOLD = 0.5                      # two unique k-mers: min_kmers = 1
BLOCK, WORD = 256, 64                # threads of a K4 workgroup = words of an item; columns of a word
CAPACITY = 1 << 16                   # entries the device lists start with
MODES = ("exact", "thr")
_LUT = np.frombuffer(b"ACGT", np.uint8)

# the pattern menu, cycled over the queries of a case ("last" right in front of "first": a query that ends in a hit followed by one
# that starts with one)
MENU = ("empty", "all", "last", "first", "cuts", "word", "second", "half", "short")
DENSE = ("all", "word", "second", "half")     # (and "short" in a thresholded run: a query without k-mers hits every column with count 0)


def plan_hits(nchunks, n_shards=1):
    """(items per group, groups, single-workgroup body): the rule of bigsi_launch.hpp, restated"""
    if nchunks == 0:
        return 1, 1, n_shards == 1
    ipb = nchunks if nchunks <= 16 else -(-nchunks // 1024)
    groups = -(-nchunks // ipb)
    return ipb, groups, groups == 1 and n_shards == 1


def export_spec(n_seqs, capacity):
    return min(max(1024, 16 * n_seqs), capacity, 1 << 20)


def min_kmers(u, thr):
    return max(int(math.ceil(u * thr)), 0)


# --------------------------------------------------------------------------------------------- shapes and cuts
def shape_of(c, n_queries):
    """what K4 sees of a call of n_queries queries: words and chunks of a result vector, shards, items and the plan"""
    width = c["shard_cols"] if c["kind"] == "group" else c["n_cols"]
    wv = -(-width // WORD)
    chunks = -(-wv // BLOCK)
    shards = len(c["devices"]) if c["kind"] == "group" else 1
    items = n_queries * shards * chunks
    ipb, groups, single = plan_hits(items, shards)
    return dict(width=width, wv=wv, chunks=chunks, shards=shards, items=items, ipb=ipb, groups=groups, single=single)


def word_cuts(c):
    """the word indices w of a case's "cuts" pattern (last column of word w - 1 + first column of word w), by name: the thread cuts
    chunks x t of the single-workgroup body, the chunk cuts 256 x c, and for a device group the first word of every shard (in words
    of the whole index).  A group cut of the general body is an item boundary: a chunk cut inside a query, or the boundary between
    two queries, which the menu's ("last", "first") neighbours straddle."""
    s = shape_of(c, c["per_call"])
    if c["kind"] == "group":
        return {"shard": [sh * c["shard_cols"] // WORD for sh in range(1, s["shards"]) if sh * c["shard_cols"] < c["n_cols"]]}
    wv = -(-c["n_cols"] // WORD)
    cuts = {"chunk": [BLOCK * i for i in range(1, s["chunks"])]}
    if s["single"]:
        cuts["thread"] = [s["chunks"] * t for t in range(1, BLOCK) if s["chunks"] * t < wv]
    return cuts


def pattern_columns(c, what, rng):
    """the columns (ascending, unique, int64) of a named pattern of the menu, or of ("first_n", T) / ("scatter_n", T) / ("cols", [..])"""
    n = c["n_cols"]
    wv = -(-n // WORD)
    if isinstance(what, tuple):
        kind, arg = what
        if kind == "first_n":
            return np.arange(arg, dtype=np.int64)
        if kind == "scatter_n":          # T columns spread over the whole width, the first and the last column among them
            cols = np.unique(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=arg - 2, replace=False)]))
            assert cols.size == arg
            return cols.astype(np.int64)
        assert kind == "cols"
        return np.unique(np.asarray(arg, np.int64))
    if what in ("empty", "short"):
        return np.zeros(0, np.int64)
    if what == "all":
        return np.arange(n, dtype=np.int64)
    if what == "first":
        return np.array([0], np.int64)
    if what == "last":
        return np.array([n - 1], np.int64)
    if what == "cuts":
        ws = sorted({w for ws_ in word_cuts(c).values() for w in ws_}) or [max(wv // 2, 1)]
        cols = np.array([x for w in ws for x in (WORD * w - 1, WORD * w)], np.int64)
        return np.unique(cols[(cols >= 0) & (cols < n)])
    if what == "word":                   # one hit per word, at a column that walks through the word
        cols = WORD * np.arange(wv, dtype=np.int64) + (7 * np.arange(wv, dtype=np.int64) + 3) % WORD
        cols[-1] = min(cols[-1], n - 1)
        return np.unique(cols)
    if what == "second":
        return np.arange(0, n, 2, dtype=np.int64)
    assert what == "half", what
    return np.flatnonzero(rng.random(n) < 0.5).astype(np.int64)


def is_dense(what, mode):
    return what in DENSE or (what == "short" and mode == "thr")


def menu_patterns(n_queries, mode, dense_cycles=1, menu=MENU):
    """the menu cycled over n_queries queries; from cycle `dense_cycles` on a dense pattern gives way to "cuts", so that a case's total
    stays what the case wants it to be"""
    out = []
    for i in range(n_queries):
        what = menu[i % len(menu)]
        out.append("cuts" if (is_dense(what, mode) and i // len(menu) >= dense_cycles) else what)
    return out


# --------------------------------------------------------------------------------------------- the cases
def _case(name, kind, n_cols, patterns, per_call=None, h=1, devices=None, run_kw=None, seed=1, note=""):
    """patterns: mode -> list of pattern names, one per query.  per_call: queries per call (default: all in one call); the calls are
    consecutive slices, or for per_call = 2 every pair of neighbours (each pattern comes first and second)."""
    c = dict(name=name, kind=kind, n_cols=n_cols, patterns=patterns, h=h, devices=devices, run_kw=run_kw or {}, seed=seed, note=note)
    if devices:
        c["shard_cols"] = -(-(-(-n_cols // len(devices))) // WORD) * WORD          # the group's rule: ceil(cols / shards) in whole words
    c["per_call"] = per_call or len(patterns("exact"))
    return c


def _menu(mode):
    return list(MENU)


def _totals(kind):
    return [(kind, t) for t in (1023, 1024, 1025, 65535, 65536, 65537)]


CASES = [
    # ---- ONE query per call through the one-call search: the menu, a call per pattern, one workspace
    _case("one_100", "one_call", 100, _menu, per_call=1, note="two words, the second ragged"),
    _case("one_16384", "one_call", 16384, _menu, per_call=1, note="one chunk, one word per thread"),
    _case("one_16385", "one_call", 16385, _menu, per_call=1, note="two chunks, a ragged last word of one bit"),
    _case("one_70016", "one_call", 70016, _menu, per_call=1, note="five chunks; 'all' overflows the lists, the rest follow in the grown workspace"),
    _case("one_262144", "one_call", 262144, _menu, per_call=1, note="16 chunks: the last shape of the single-workgroup body"),
    _case("one_262145", "one_call", 262145, lambda mode: list(MENU) + [("first_n", t) for t in (1023, 1024, 1025)], per_call=1,
          note="17 items: the general body and k_export_results; totals on the export's size"),
    # ---- totals on the export's size (1024) and on the lists' capacity (65 536), a small call behind the overflow
    _case("totals_first", "one_call", 70016, lambda mode: _totals("first_n") + ["cuts", "first"], per_call=1),
    _case("totals_scattered", "one_call", 70016, lambda mode: _totals("scatter_n") + ["cuts", "last"], per_call=1),
    # ---- two queries per call: 16 items (the single-workgroup body with two queries) and 18 (two queries cannot make 17: items =
    # queries x chunks); 17 queries of one chunk make 17
    _case("two_16", "one_call", 131072, _menu, per_call=2, note="2 x 8 chunks"),
    _case("two_18", "one_call", 131073, _menu, per_call=2, note="2 x 9 chunks"),
    _case("seventeen", "one_call", 16347, lambda mode: menu_patterns(17, mode), note="17 x 1 chunk in one call"),
    # ---- batches through new_batch / run / hits
    _case("b1024", "batch", 16347, lambda mode: menu_patterns(1024, mode), note="1024 items, ipb 1"),
    _case("b1025", "batch", 16347, lambda mode: menu_patterns(1025, mode), note="1025 items, ipb 2, a last group of one; groups straddle queries"),
    _case("b700x3", "batch", 40000, lambda mode: menu_patterns(700, mode), note="2100 items, ipb 3: a group is a query"),
    _case("b400x3", "batch", 40000, lambda mode: menu_patterns(400, mode), note="1200 items, ipb 2: groups cut inside queries"),
    _case("b_last_only", "batch", 16347, lambda mode: ["empty"] * 299 + ["all"], note="300 groups, hits only in the last query"),
    _case("b_first_only", "batch", 16347, lambda mode: ["all"] + ["empty"] * 299, note="300 groups, hits only in the first query"),
    _case("b_sparse", "batch", 16347, lambda mode: menu_patterns(1025, mode), run_kw=dict(sparse_counts=True), note="b1025 with sparse counts"),
    _case("b_regrow", "batch", 16347, lambda mode: [("all" if i in (100, 200, 300, 400, 500) else w) for i, w in enumerate(menu_patterns(600, mode, dense_cycles=0))],
          note="600 groups; the total passes 65 536 inside query 400: regrow + write_only"),
    # ---- reads: k_reads_fused + k_export_reads (h = 2, 128 columns), one call each
    _case("r1", "reads", 128, lambda mode: [w for w in MENU if w != "short"], per_call=1, h=2, note="one read per call: the read kernel exports inline"),
    _case("r257", "reads", 128, lambda mode: menu_patterns(257, mode), h=2, note="two workgroups of k_export_reads"),
    _case("r16400", "reads", 128, lambda mode: menu_patterns(16400, mode), h=2, note="64 workgroups x 257 queries: the re-ordering loop runs twice"),
    _case("r300_all", "reads", 128, lambda mode: ["all"] * 300, h=2, note="38 400 hits > exp_spec 4800: the host re-orders"),
    _case("r_spec", "reads", 128, lambda mode: ["all"] * 8 + [("first_n", 16)] + ["empty"] * 56, h=2, note="65 reads, total == exp_spec == 1040"),
    _case("r_spec1", "reads", 128, lambda mode: ["all"] * 8 + [("first_n", 17)] + ["empty"] * 56, h=2, note="65 reads, total == exp_spec + 1"),
    # ---- a device group of three shards on one device: 1000 columns in shards of 384, 384 and 232
    _case("g2", "group", 1000, lambda mode: ["cuts", ("cols", [0, 383, 768, 999])], devices=[0, 0, 0], note="6 items in one group of the general body; shard 1 without hits in query 1"),
    _case("g20", "group", 1000, lambda mode: menu_patterns(18, mode) + [("cols", [0, 383, 768, 999]), ("cols", [384, 767])], devices=[0, 0, 0], note="60 items"),
    _case("g400", "group", 1000, lambda mode: menu_patterns(398, mode) + [("cols", [0, 383, 768, 999]), ("cols", [384, 767])], devices=[0, 0, 0],
          note="1200 items, ipb 2: groups straddle shards and queries"),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
PARAMS = [(c["name"], mode) for c in CASES for mode in MODES]


class Built(object):
    """One case in one mode.  Attributes: case, mode, threshold, queries (str), patterns, row_ids (uint64, ascending), packed
    (uint8[rows, ceil(n_cols / 8)]), m, calls (lists of query indices)."""

    def __init__(self, c, mode):
        self.case, self.mode = c, mode
        self.threshold = 1.0 if mode == "exact" else THRESHOLD
        self.patterns = c["patterns"](mode)
        n, h, n_cols = len(self.patterns), c["h"], c["n_cols"]
        per = c["per_call"]
        self.calls = [[i, i + 1] for i in range(n - 1)] if per == 2 else [list(range(i, min(i + per, n))) for i in range(0, n, per)]
        kmers = 1 if mode == "exact" else 2
        self.m = max(1009, 4 * n * kmers * h + 1)
        rng = np.random.default_rng(c["seed"] * 1000 + MODES.index(mode))
        self.queries, ids, rows_bits, taken = [], [], [], set()
        for what in self.patterns:
            cols = pattern_columns(c, what, rng)
            while True:
                length = 20 if what == "short" else K - 1 + kmers
                seq = _LUT[rng.integers(0, 4, size=length)].tobytes().decode("ascii")
                rows = coracle.seq_rows(seq, K, h, self.m)
                flat = [int(r) for r in rows.ravel()]
                if len(coracle.unique_kmers(seq, K)[0]) == rows.shape[0] and len(set(flat)) == len(flat) and not taken & set(flat):
                    break
            taken |= set(flat)
            self.queries.append(seq)
            for j in range(rows.shape[0]):
                mine = cols if kmers == 1 else cols[cols % 3 != (2 if j == 0 else 1)]
                mask = np.zeros(n_cols, bool)
                mask[mine] = True
                bits = np.packbits(mask)
                for r in rows[j]:
                    ids.append(int(r))
                    rows_bits.append(bits)
        order = np.argsort(np.array(ids, np.uint64), kind="stable")
        self.row_ids = np.array(ids, np.uint64)[order]
        self.packed = np.stack(rows_bits)[order] if ids else np.zeros((0, (n_cols + 7) // 8), np.uint8)
        assert np.unique(self.row_ids).size == self.row_ids.size
        self._ref = None

    # ---- the reference
    def counts(self, seq):
        """(positions, u, int64[n_cols]) of any sequence against the rows written"""
        c = self.case
        first, _ = coracle.unique_kmers(seq, K)
        counts = np.zeros(c["n_cols"], np.int64)
        nk = max(len(seq) - K + 1, 0)
        if len(first) == 0:
            return nk, 0, counts
        rows = coracle.seq_rows(seq, K, c["h"], self.m)[first]
        idx = np.minimum(np.searchsorted(self.row_ids, rows), self.row_ids.size - 1)
        idx = idx[(self.row_ids[idx] == rows).all(axis=1)]          # a k-mer with a row that was never written counts nowhere
        for one in idx:
            a = self.packed[one[0]].copy()
            for j in one[1:]:
                a &= self.packed[j]
            counts += np.unpackbits(a)[:c["n_cols"]]
        return nk, len(first), counts

    def reference(self):
        """per query (nk, u, mk, colours uint32, counts uint32); computed once, shared, never changed"""
        if self._ref is None:
            out = []
            for seq in self.queries:
                nk, u, counts = self.counts(seq)
                mk = min_kmers(u, self.threshold)
                hit = (counts == u) if self.mode == "exact" else (counts >= mk)
                cols = np.flatnonzero(hit) if (u > 0 or self.mode == "thr") else np.zeros(0, np.int64)
                col, cnt = cols.astype(np.uint32), counts[cols].astype(np.uint32)
                col.setflags(write=False)
                cnt.setflags(write=False)
                out.append((nk, u, mk, col, cnt))
            self._ref = out
        return self._ref

    def expected(self, call):
        """(nk, nu, mk, off uint64[n + 1], colours, counts) of a call"""
        ref = [self.reference()[q] for q in call]
        off = np.concatenate([[0], np.cumsum([r[3].size for r in ref])]).astype(np.uint64)
        cat = lambda i: np.concatenate([r[i] for r in ref]) if ref else np.zeros(0, np.uint32)          # noqa: E731
        return (np.array([r[0] for r in ref], np.uint32), np.array([r[1] for r in ref], np.uint32), np.array([r[2] for r in ref], np.uint32),
                off, cat(3), cat(4))

    # ---- the paths
    def paths(self):
        """per call what bigsi_hip_hits_last_path must report, and the capacity of the device lists before the call"""
        c, ref = self.case, self.reference()
        one_call = c["kind"] in ("one_call", "reads")
        cap, out = CAPACITY, []
        for call in self.calls:
            if not one_call:
                cap = CAPACITY          # a batch object of its own
            total = sum(ref[q][3].size for q in call)
            s = shape_of(c, len(call))
            fused = c["kind"] == "reads"
            assert not fused or sum(ref[q][0] for q in call) > 0, "a read call without a k-mer does not take the read kernel"
            spec = export_spec(len(call), cap) if one_call else 0
            over = total > cap
            out.append(dict(groups=0 if fused else s["groups"], items_per_group=0 if fused else s["ipb"],
                            single_workgroup=int(s["single"] and not fused),
                            inline_export=int(one_call and (len(call) == 1 if fused else s["single"])),
                            rewrites=int(over), exp_spec=spec, collect_fetch=int(one_call and (over or (fused and total > spec))),
                            one_launch=int(fused), capacity_before=cap, total=total))
            cap = max(cap, total)
        return out


_built = {}


def build_case(name, mode):
    """built once per process and shared; nobody changes it"""
    if (name, mode) not in _built:
        _built[(name, mode)] = Built(CASE_BY_NAME[name], mode)
    return _built[(name, mode)]
