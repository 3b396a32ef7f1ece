"""The "staircase" index of the counting tests (a plain module: nothing here is collected): for ONE main query an index whose
per-column counts are chosen, not drawn -- 0, 1, u - 1, u, both sides of every power of two and of every threshold -- built on the host
from numpy and oracle.coracle alone, with its numpy reference, and the table of cases (CASES) that tests/test_count_staircase_host.py
pins on the CPU and tests/test_gpu_count_planes.py runs on the device.

Method.  The main sequence has u unique k-mers (k = 31) in first-occurrence order, each with h rows.  Column c "holds" k-mer j when
all h rows of j have bit c set; a column holds a prefix of one of three orders of the k-mers -- EARLY: the k-mer order itself, LATE:
the order reversed (a suffix), SCATTERED: a seeded permutation.  Rows collide, so a column's count (the k-mers ALL of whose rows have
the bit) is not the length of its prefix: it is monotone in that length, and the length is bisected until the count is the target.
A target the bisection cannot hit (the count jumps over it) raises: no case leaves a target out; another seed does it.
Only the touched rows are written; every other row of the index stays zero.  reference(seq) counts any sequence against the rows
written: sum over its unique k-mers of the AND over the k-mer's h rows, a k-mer with an untouched row contributing nothing.  Filler
queries are substrings of the main sequence and get varied counts from the same columns."""
import math

import numpy as np

from oracle import coracle

K = 31
FAMILIES = ("early", "late", "scattered")
_LUT = np.frombuffer(b"ACGT", np.uint8)


def min_kmers(u, thr):
    """ceil(u * threshold) in IEEE double, as graph/bigsi.py:179 and K1 evaluate it"""
    return max(int(math.ceil(u * thr)), 0)


def threshold_for(u, mk):
    """a threshold with ceil(u * thr) == mk (mk >= 1)"""
    thr = (mk - 0.5) / u
    assert min_kmers(u, thr) == mk
    return thr


def make_main(positions, seed, dup=2):
    """A random sequence of `positions` k-mer positions with one internal repeat: `dup` k-mers of its first third come back in its
    last third (short sequences: the first k-mers come back at the end), so that u < positions and first-occurrence order matters."""
    rng = np.random.default_rng(seed)
    s = _LUT[rng.integers(0, 4, size=positions + K - 1)].copy()
    if positions > dup:
        a, b = positions // 3, 2 * positions // 3
        if b - a < K + dup:
            a, b = 0, positions - dup
        for i in range(K - 1 + dup):          # (left to right: an overlapping copy makes the stretch periodic)
            s[b + i] = s[a + i]
    return s.tobytes().decode("ascii")


def unique_count(seq):
    return len(coracle.unique_kmers(seq, K)[0])


def auto_thresholds(u):
    """Two thresholds of a main query of u unique k-mers: min_kmers a power of two, and one less (all ones below a plane)."""
    mk = 1 << int(math.floor(math.log2(max(u - 1, 2))))
    return [threshold_for(u, mk), threshold_for(u, mk - 1)]


def targets_for(u, mks):
    t = {0, 1, u - 1, u}
    p = 0
    while (1 << p) - 1 <= u:
        t.add((1 << p) - 1)
        if (1 << p) <= u:
            t.add(1 << p)
        p += 1
    for mk in mks:
        t.update(x for x in (mk - 1, mk, mk + 1) if 0 <= x <= u)
    return sorted(x for x in t if 0 <= x <= u)


def edge_columns(n_cols, tile_words=(), lo=0):
    """The named edge columns of [lo, n_cols): both ends of the first two words, the last column, the first column of the last word,
    and at every tile cut (a word index) both ends of the word before it and the first column behind it."""
    wv = -(-n_cols // 64)
    e = {lo, lo + 63, lo + 64, lo + 127, n_cols - 1, 64 * (wv - 1)}
    for b in tile_words:
        e.update((64 * (b - 1), 64 * b - 1, 64 * b))
    return sorted(c for c in e if lo <= c < n_cols)


def filler_positions(n, fmax):
    """k-mer positions of n filler queries, at most fmax each: some below 10, some below 96, one sequence shorter than k (-1), and
    from the ninth on a walk that takes every residue mod 8."""
    head = [9, 95, -1, 3, 40, 62, 8, 21]
    out = [min(p, fmax) for p in head[:n]]
    step = 37 if fmax % 37 else 41
    out += [1 + (i * step) % fmax for i in range(len(out), n)]
    return out


def make_fillers(main, n, fmax, seed):
    rng = np.random.default_rng(seed + 1)
    out = []
    for p in filler_positions(n, fmax):
        length = 20 if p < 0 else p + K - 1
        a = int(rng.integers(0, len(main) - length + 1))
        out.append(main[a:a + length])
    return out


class Staircase(object):
    """The staircase of one main sequence.  Attributes: u, thresholds, mks (min_kmers of the main per threshold), targets, columns
    (list of (column, target, family); `columns=` gives them instead of the general staircase), edges (the named edge columns), row_ids (uint64, ascending) and packed (uint8[rows,
    ceil(n_cols / 8)]): the rows to write."""

    def __init__(self, s, h, m, n_cols, thresholds, seed, tile_words=(), late_from=None, columns=None):
        self.main, self.h, self.m, self.n_cols, self.seed = s, h, m, n_cols, seed
        first, _ = coracle.unique_kmers(s, K)
        self.u = u = len(first)
        assert 1 <= u < len(s) - K + 1, "the main sequence needs an internal repeat"
        krows = coracle.seq_rows(s, K, h, m)[first]                     # [u, h], first-occurrence order
        self.row_ids = np.unique(krows)
        self.kidx = np.searchsorted(self.row_ids, krows)                 # the same, as indices into row_ids
        self.thresholds = list(thresholds)
        self.mks = [min_kmers(u, t) for t in self.thresholds]
        self.targets = targets_for(u, self.mks)
        self.packed = np.zeros((self.row_ids.size, (n_cols + 7) // 8), np.uint8)
        rng = np.random.default_rng(seed)
        orders = {"early": np.arange(u), "late": np.arange(u)[::-1].copy(), "scattered": rng.permutation(u)}
        done = {f: self._completion(orders[f]) for f in FAMILIES}
        if columns is not None:
            # the caller's own columns instead of the general staircase (tests/rank_cases.py): placed by the same bisection
            self.columns = [(int(c), int(t), f) for c, t, f in columns]
            self.edges = sorted(c for c, _, _ in self.columns)
            assert len(set(self.edges)) == len(self.edges) and 0 <= self.edges[0] and self.edges[-1] < n_cols and late_from is None
            self._place(orders, done)
            return

        # the general staircase lies in [0, hi); with late_from the columns from there on hold late-family columns at mk - 1 and mk only
        hi = n_cols if late_from is None else late_from
        self.edges = edge_columns(hi, tile_words)
        entries = [(t, f) for t in self.targets for f in FAMILIES]
        assert len(entries) <= hi, "more staircase columns than columns"
        # the edge columns take the most telling targets: around the thresholds, then u, u - 1, then the powers of two downwards
        telling = [t for mk in self.mks for t in (mk, mk - 1, mk + 1)] + [u, u - 1] + self.targets[::-1]
        telling = [t for i, t in enumerate(telling) if t > 0 and t in self.targets and t not in telling[:i]]
        front = [(t, FAMILIES[i % 3]) for i, t in enumerate(telling)][:len(self.edges)]
        assert len(front) == len(self.edges)
        rest = [e for e in entries if e not in front]
        free = np.setdiff1d(np.arange(hi), self.edges)
        where = list(self.edges) + sorted(rng.choice(free, size=len(rest), replace=False).tolist())
        self.columns = [(c, t, f) for c, (t, f) in zip(where, front + rest)]
        if late_from is not None:
            self.late_edges = edge_columns(n_cols, (), lo=late_from)
            late_t = sorted({t for mk in self.mks for t in (mk - 1, mk)})
            self.columns += [(c, late_t[i % len(late_t)], "late") for i, c in enumerate(self.late_edges)]
            self.edges = self.edges + self.late_edges
        self._place(orders, done)

    def _place(self, orders, done):
        for c, t, f in self.columns:
            length = self._bisect(done[f], t)
            rows = np.unique(self.kidx[orders[f][:length]])
            self.packed[rows, c >> 3] |= np.uint8(0x80 >> (c & 7))

    def _completion(self, order):
        """For every k-mer the length of the prefix of `order` from which on a column holds it: all of its rows are then set, by
        itself or by the rows of others."""
        u = self.u
        first_set = np.full(self.row_ids.size, u, np.int64)
        np.minimum.at(first_set, self.kidx[order].ravel(), np.repeat(np.arange(u), self.h))
        return first_set[self.kidx].max(axis=1) + 1

    def _bisect(self, done, t):
        """The shortest prefix whose column counts at least t k-mers -- and then exactly t, or the seed misses the target."""
        lo, hi = 0, self.u
        while lo < hi:
            mid = (lo + hi) // 2
            if np.count_nonzero(done <= mid) >= t:
                hi = mid
            else:
                lo = mid + 1
        if np.count_nonzero(done <= lo) != t:
            raise ValueError("seed %d misses the target %d (u = %d): take another seed" % (self.seed, t, self.u))
        return lo

    def reference(self, seq):
        """(u, counts int64[n_cols]) of any sequence against the rows written"""
        first, _ = coracle.unique_kmers(seq, K)
        counts = np.zeros(self.n_cols, np.int64)
        if len(first) == 0:
            return 0, counts
        rows = coracle.seq_rows(seq, K, self.h, self.m)[first]
        idx = np.minimum(np.searchsorted(self.row_ids, rows), self.row_ids.size - 1)
        idx = idx[(self.row_ids[idx] == rows).all(axis=1)]
        step = max(1, (32 << 20) // (8 * self.packed.shape[1]))
        for i in range(0, idx.shape[0], step):
            a = self.packed[idx[i:i + step, 0]]
            for j in range(1, self.h):
                a &= self.packed[idx[i:i + step, j]]
            counts += np.unpackbits(a, axis=1)[:, :self.n_cols].sum(axis=0, dtype=np.int64)
        return len(first), counts

    def dense(self):
        """the whole index, uint8[m, ceil(n_cols / 8)]"""
        out = np.zeros((self.m, self.packed.shape[1]), np.uint8)
        out[self.row_ids.astype(np.int64)] = self.packed
        return out


# --------------------------------------------------------------------------------------------- the cases
# The smallest shapes that take each route of the counting path.  `route` is what the launch planner (bigsi_launch.hpp) answers for
# the batch: the host test asks the compiled planner and a case that moves off its route fails there.  n_cols = 200 is 4 result words,
# the last one ragged.  A batch is the main query followed by n_queries - 1 fillers of at most `fmax` positions.
SMALL_M, MID_M, LARGE_M = 20011, 200003, 1000003


def _route(P, slices, planes_out=0, block=256, tiles=1, deep=0, early=0):
    return dict(P=P, count_bytes=2 if P <= 16 else 4, slices=slices, planes_out=planes_out, combine=int(slices > 1), deep=deep, early=early,
                block=block, tiles=tiles)


def _case(name, main_pos, route, n_queries=1, h=3, m=None, n_cols=200, fmax=150, sparse=False, early=False, one_launch=0, seed=1, **kw):
    return dict(name=name, main_pos=main_pos, route=route, n_queries=n_queries, h=h, m=m or (LARGE_M if main_pos > 4096 or h == 1 else MID_M if main_pos > 2048 else SMALL_M),
                n_cols=n_cols, fmax=min(fmax, main_pos), sparse=sparse, early=early, one_launch=one_launch, seed=seed, **kw)


_P_OF = {63: 6, 1023: 10, 1024: 12, 4096: 16, 65570: 32}
CASES = [
    # one query, sliced: k_and_count leaves `planes_out` planes per slice, k_count_combine adds them up (<= 4 planes: its fast path)
    _case("S6", 63, _route(6, 6, 4)),
    _case("S10", 64, _route(10, 6, 4)),
    _case("S10b", 1023, _route(10, 96, 4)),
    _case("S12", 1024, _route(12, 96, 4)),
    _case("S12b", 4095, _route(12, 96, 6)),
    _case("S16", 4096, _route(16, 96, 6)),
    _case("S16b", 65535, _route(16, 96, 10), n_cols=400),
    _case("S32", 65570, _route(32, 96, 10), n_cols=400),
    # sliced, with queries that leave slices without k-mers (live < slices)
    _case("Smix", 4096, _route(16, 96, 6), n_queries=9, fmax=95),
    # a one-query batch that is one slice
    _case("Sone", 9, _route(6, 1)),
]
# one slice (>= 1024 wavefronts), 4-wavefront workgroups
CASES += [_case("Uplain%d" % _P_OF[p], p, _route(_P_OF[p], 1), n_queries=1024) for p in (63, 1023, 1024, 4096, 65570)]
# one slice in one-wavefront workgroups and the software-pipelined loop (KMX = 2; it exists for h = 3 and 4)
CASES += [_case("Udeep%d_h%d" % (_P_OF[p], h), p, _route(_P_OF[p], 1, block=64, deep=1), n_queries=1030, h=h)
          for p in (1024, 4096, 65570) for h in (3, 4)]
CASES += [
    _case("Usparse10", 1023, _route(10, 1), n_queries=1024, sparse=True),
    _case("Usparse16", 4096, _route(16, 1, block=64, deep=1), n_queries=1030, sparse=True),
    # early exit: two wavefronts per query, the second one's columns all late-family at mk - 1 and mk
    _case("Uearly", 1024, _route(12, 1, block=64, tiles=2, early=1), n_queries=520, n_cols=8192 + 136, sparse=True, early=True, late_from=8192),
    # 513 words: the last lane's second word lies beyond the result
    _case("Wide64", 1024, _route(12, 1, block=64, tiles=5, deep=1), n_queries=205, n_cols=32832, fmax=60, tile_words=(128, 256, 384, 512)),
    _case("Wide256", 1100, _route(12, 1, block=256, tiles=2), n_queries=640, n_cols=32832, fmax=60, tile_words=(128, 256, 384, 512)),
]
# the H = 1, 2, 5 instances and the run-time-h loop
CASES += [_case("S10b_h%d" % h, 1023, _route(10, 96, 4), h=h) for h in (1, 2, 5, 7)]
CASES += [_case("Uplain10_h%d" % h, 1023, _route(10, 1), n_queries=1024, h=h) for h in (1, 2, 5, 7)]
# reads: k_reads_fused (one launch; the planner is not asked) -- a handful of reads (the split workgroup), one word per lane, two
CASES += [_case("R%s_h%d" % (kind, h), 63, None, n_queries=n, h=h, n_cols=n_cols, sparse=True, one_launch=1)
          for kind, n, n_cols in (("split", 40, 200), ("narrow", 300, 200), ("two", 300, 20000)) for h in (2, 3, 4)]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

_built = {}


def build_case(name):
    """(case, staircase, queries): built once per process and shared; nobody changes them."""
    if name not in _built:
        c = CASE_BY_NAME[name]
        main = make_main(c["main_pos"], c["seed"])
        sc = Staircase(main, c["h"], c["m"], c["n_cols"], auto_thresholds(unique_count(main)), c["seed"],
                       tile_words=c.get("tile_words", ()), late_from=c.get("late_from"))
        _built[name] = (c, sc, [main] + make_fillers(main, c["n_queries"] - 1, c["fmax"], c["seed"]))
    return _built[name]
