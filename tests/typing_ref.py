"""Support shared by tests/test_typing_host.py and tests/test_gpu_typing.py (a plain module: nothing here is collected): the numpy
reference of the locus typing (include/bigsi_hip_typing.h) over tally_ref's planted indexes -- `us` and `counts` come from the
finished matrix, never from the plan --, the scheme the cases use and its record layouts, a plain Python restatement of the host
planner plan_typing (csrc/bigsi_launch.hpp) that the host test pins against the compiled header, and the conditions the cases must
hold so that a GPU comparison cannot pass emptily.

The planted index (tally_ref): M = 40009, H = 3, K = 31; query i is planted whole into edge column e_j when (i + j) % 3 == 0 and by
half when it is 1; query 1 hits nothing and query 2 is shorter than k.

The scheme over n planted queries, 24 loci with records and two without (N_LOCI = 26).  Query i < 48 is a record of locus (i // 2)
% 24 -- neighbours share a locus --, query i >= 48 of locus (i - 48) % 24: a locus then has records 48 or more apart, in different
tiles of k_locus_best from record 64 on.  The identity of query i is 64 - i: later records have LOWER identities, so "the first hit
wins" and "the lowest identity wins" are different answers.  Loci 24 and 25 have no record.

The layouts put the same records in another order: "grouped" -- by locus, as bigsi_amd.locus_typing.parse_scheme gives them;
"interleaved" -- in query order, so that one locus's records lie in different tiles; "shuffled" -- a fixed permutation in which
every seventh record is BIGSI_TYPING_NONE (it is then in no locus: the reference follows the layout, not the scheme)."""
import numpy as np

import tally_ref as T

NONE = 0xFFFFFFFF
MAX_ALLELE = 0xFFFFFFFE
MAX_LOCI = 1 << 20
CELL_BYTES = 4 << 30
EXACT = 0xFFFFFFFF
LAYOUTS = ("grouped", "interleaved", "shuffled")
CONDITION_WIDTHS = (200, 775)
WIDTHS = (1, 63, 64, 65, 127, 129, 200, 775)
N_QUERIES = 65
LOCI_WITH_RECORDS, N_LOCI = 24, 26

# --------------------------------------------------------------------------------------------- the planner, restated
BLOCK, TILE, LOADS = 256, 64, 8


def plan_typing(n_seqs, wv, n_loci):
    word_groups, tiles = -(-wv // (BLOCK // 64)), -(-n_seqs // TILE)
    grid = min(word_groups * tiles, (1 << 64) - 1)                                    # (the grid saturates at 64 bits)
    bad = n_loci == 0 or n_loci > MAX_LOCI
    loci_grid = 0 if bad else -(-n_loci // (BLOCK // 64))
    counts_grid = 0 if bad else loci_grid + word_groups
    too_large = grid if grid > 0x7FFFFFFF else max(counts_grid, word_groups) if max(counts_grid, word_groups) > 0x7FFFFFFF else 0
    too_many = (not bad) and n_loci * wv * 768 > CELL_BYTES
    return dict(block=BLOCK, tile=TILE, word_groups=word_groups, tiles=tiles, grid=grid, loci_grid=loci_grid, words_grid=word_groups, counts_grid=counts_grid,
                cell_bytes=0 if bad or too_many else n_loci * wv * 768, too_large=too_large, bad_loci=int(bad), too_many_bytes=int(too_many))


def key_of(c, u, allele):
    """the definition, in Python integers"""
    return (int(c) * EXACT // int(u)) << 32 | (0xFFFFFFFF - int(allele))


# --------------------------------------------------------------------------------------------- the scheme and its layouts
def labels(n):
    """(locus of query i uint32[n], identity of query i uint32[n], n_loci): the scheme of the module text"""
    i = np.arange(n)
    locus = np.where(i < 48, (i // 2) % LOCI_WITH_RECORDS, (i - 48) % LOCI_WITH_RECORDS).astype(np.uint32)
    return locus, (64 - i).astype(np.uint32), N_LOCI


def layout(name, n):
    """(order int64[n]: the query at every position, locus_of uint32[n] and allele_of uint32[n] by position, n_loci)"""
    locus, allele, nl = labels(n)
    if name == "grouped":
        order = np.argsort(locus, kind="stable")
        return order, locus[order], allele[order], nl
    if name == "interleaved":
        return np.arange(n), locus.copy(), allele.copy(), nl
    if name == "shuffled":
        order = np.random.default_rng(2000 + n).permutation(n)
        lo = locus[order]
        lo[3::7] = NONE
        return order, lo, allele[order], nl
    raise KeyError(name)


def hits_of(p, thr):
    """bool[n, n_cols]: the hits a search at `thr` reports, from the definition"""
    mk = np.array([T.min_kmers(int(u), thr) for u in p.us], np.int64)
    return (p.counts >= mk[:, None]) & (p.us > 0)[:, None]


def column_mask(p):
    """A selection in the row format that drops the first edge column a record hits at threshold 1 and has every bit behind num_cols
    set (junk: it is ignored).  Returns (columns uint8[ceil(n_cols / 8)], the dropped column)."""
    hit = hits_of(p, 1.0)
    drop = next(e for e in p.edges if hit[:, e].any())
    bits = np.ones(-(-p.n_cols // 8) * 8, np.uint8)
    bits[drop] = 0
    return np.packbits(bits), drop


# --------------------------------------------------------------------------------------------- the reference
def typing_of(us, counts, hit, order, locus_of, allele_of, n_loci, columns=None):
    """dict(best uint64[n_loci, n_cols], hits uint32[n_loci, n_cols], loci uint32[n_loci, 3], samples uint32[n_cols, 2], records
    uint32[n_loci]): the definition, line by line"""
    n_cols = hit.shape[1]
    sel = np.ones(n_cols, bool) if columns is None else np.unpackbits(np.asarray(columns, np.uint8))[:n_cols].astype(bool)
    best, hits, records = np.zeros((n_loci, n_cols), np.uint64), np.zeros((n_loci, n_cols), np.uint32), np.zeros(n_loci, np.uint32)
    for pos, q in enumerate(order):
        l = int(locus_of[pos])
        if l == NONE or us[q] == 0:
            continue
        records[l] += 1
        for s in np.flatnonzero(hit[q] & sel):
            best[l, s] = max(int(best[l, s]), key_of(counts[q, s], us[q], allele_of[pos]))
            hits[l, s] += 1
    exact = (best >> np.uint64(32)) == np.uint64(EXACT)
    loci = np.stack([(best != 0).sum(axis=1), exact.sum(axis=1), (hits > 1).sum(axis=1)], axis=1).astype(np.uint32)
    samples = np.stack([(best != 0).sum(axis=0), exact.sum(axis=0)], axis=1).astype(np.uint32)
    return dict(best=best, hits=hits, loci=loci, samples=samples, records=records)


_results = {}


def planted_typing(p, thr, name, masked=False, sel=None):
    """the reference of a planted index under a layout (of its first `sel` queries, default all): computed once per process and
    shared; nobody changes it"""
    n = len(p.seqs) if sel is None else sel
    key = (id(p), thr, name, masked, n)
    if key not in _results:
        order, lo, al, nl = layout(name, n)
        _results[key] = typing_of(p.us, p.counts, hits_of(p, thr), order, lo, al, nl, column_mask(p)[0] if masked else None)
        for a in _results[key].values():
            a.setflags(write=False)
    return _results[key]


def width_case(n_cols):
    return T.planted(n_cols, N_QUERIES, seed=65)


def thresholds(p):
    """1.0 (an exact run), 0.4, a threshold whose min_kmers sits exactly on a count an edge column holds, and 0"""
    if any(0 < int(p.counts[i, e]) < u for i, u in enumerate(p.us) for e in p.edges):
        return (1.0, 0.4, p.edge_threshold()[0], 0.0)
    return (1.0, 0.4, 0.5, 0.0)


# --------------------------------------------------------------------------------------------- non-vacuity
def census(p, thr, name="grouped"):
    """What the cells of a case hold, from the definition alone -- per (locus, column) over the records that hit it: dict(called,
    not_lowest: the winner is not the lowest identity among them, ties: two or more of them share the top score (the winner is then
    the lowest identity of those), partial: the winner's score is below 2^32 - 1, multiple: hits > 1, scores: the distinct scores)"""
    order, lo, al, nl = layout(name, len(p.seqs))
    hit = hits_of(p, thr)
    out = dict(called=0, not_lowest=0, ties=0, partial=0, multiple=0, empty=0, scores=set())
    for l in range(nl):
        pos = [i for i in range(len(order)) if lo[i] == l and p.us[order[i]] > 0]
        for s in range(p.n_cols):
            mine = [(int(p.counts[order[i], s]) * EXACT // int(p.us[order[i]]), int(al[i])) for i in pos if hit[order[i], s]]
            if not mine:
                out["empty"] += 1
                continue
            top = max(sc for sc, _ in mine)
            winner = min(a for sc, a in mine if sc == top)
            out["called"] += 1
            out["not_lowest"] += winner != min(a for _, a in mine)
            out["ties"] += sum(sc == top for sc, _ in mine) > 1
            out["partial"] += top < EXACT
            out["multiple"] += len(mine) > 1
            out["scores"].add(top)
    return out


def two_tile_locus(name, n):
    """(locus, position 1, position 2) of a locus whose records lie in two different tiles of k_locus_best under the layout, or None"""
    _, lo, _, _ = layout(name, n)
    first = {}
    for pos, l in enumerate(lo.tolist()):
        if l == NONE:
            continue
        if first.setdefault(l, pos) // TILE != pos // TILE:
            return l, first[l], pos
    return None


def check_conditions(p, thr):
    """What a width case must hold at threshold `thr` so that a comparison against planted_typing cannot pass emptily."""
    assert len(p.seqs) == N_QUERIES > TILE
    g = planted_typing(p, thr, "grouped")
    c = census(p, thr)
    assert c["called"] == int((g["best"] != 0).sum()) and c["multiple"] == int((g["hits"] > 1).sum()) and c["partial"] == int(g["loci"][:, 0].sum() - g["loci"][:, 1].sum())
    assert c["ties"] >= 1, "no tie at the top score: the lowest-identity rule decides nothing"
    assert c["multiple"] >= 1 and c["empty"] >= 1, "no cell with hits >= 2, or no empty cell"
    assert not g["records"][LOCI_WITH_RECORDS:].any() and not g["best"][LOCI_WITH_RECORDS:].any() and (g["records"][:LOCI_WITH_RECORDS] > 0).all(), "loci without records"
    assert two_tile_locus("interleaved", len(p.seqs)) is not None and two_tile_locus("grouped", len(p.seqs)) is not None
    if thr < 1.0:
        assert c["not_lowest"] >= 1, "every winner is the lowest identity among its hits: a min over identities would pass"
        assert c["partial"] >= 1 and len(c["scores"]) >= 3, "no winner with a partial score: the counters decide nothing"
    else:
        assert c["partial"] == 0 and c["not_lowest"] == 0          # (an exact run: every hit has c = u)
    # grouped and interleaved are the same scheme: the same reference; the shuffled layout's NONE entries take records away
    a = planted_typing(p, thr, "interleaved")
    assert all(np.array_equal(a[k], g[k]) for k in g)
    assert not np.array_equal(planted_typing(p, thr, "shuffled")["records"], g["records"])
    # the mask drops a column that is called without it
    columns, drop = column_mask(p)
    m = planted_typing(p, thr, "grouped", masked=True)
    assert g["best"][:, drop].any() and not m["best"][:, drop].any() and not m["hits"][:, drop].any() and not m["samples"][drop].any()
    return c
