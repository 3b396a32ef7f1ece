"""Support shared by tests/test_genotype_host.py and tests/test_gpu_genotype.py (a plain module: nothing here is collected): the numpy
reference of the panel genotyping (include/bigsi_hip_genotype.h) over tally_ref's planted indexes -- `us` and `counts` come from the
finished matrix, never from the plan --, the panel the cases use and its probe layouts, a plain Python restatement of the host planner
plan_genotype (csrc/bigsi_launch.hpp) that the host test pins against the compiled header, and the conditions the cases must hold so
that a GPU comparison cannot pass emptily.

The planted index (tally_ref): M = 40009, H = 3, K = 31; query i is planted whole into edge column e_j when (i + j) % 3 == 0 and by
half when it is 1; query 1 hits nothing and query 2 is shorter than k.

The panel over n planted queries, V = 24 paired variants and four special ones (alleles()).  Query i goes by c = i % 48: c < 24 is a
ref probe of variant c; otherwise c' = c - 24 is an alt probe, of variant c' when c' is even and of variant (c' - 2) % 24 when it is
odd.  24 = 0 (mod 3), so an even variant's ref and alt probes hit the SAME edge columns (0/1 there, missing elsewhere) and an odd
variant's hit DIFFERENT ones (0/0 at one, 1/1 at another).  From 48 queries on a variant has two ref probes, 48 apart: in different
tiles of k_allele_or from probe 64 on.  The special variants take four queries out of that: ALT_ONLY (24) has query 5 as its only
probe, NO_ALT (25) query 8 as its only probe, a ref; EMPTY (26) has no probe at all -- missing everywhere, at every threshold --; and
SHORT_ALT (27) has query 11 as ref and the short query 2 as its only alt probe: used[27][1] == 0.

The layouts put the same probes in another order: "grouped" -- by allele, as bigsi_amd.genotype.parse_panel gives them;
"interleaved" -- in query order, so that one allele's probes lie 48 apart; "shuffled" -- a fixed permutation in which every seventh
probe is BIGSI_GENOTYPE_NONE (it is then in no allele: the reference follows the layout, not the panel)."""
import numpy as np

import tally_ref as T

NONE = 0xFFFFFFFF
MAX_VARIANTS = 1 << 20
PLANE_BYTES = 4 << 30
LAYOUTS = ("grouped", "interleaved", "shuffled")
CONDITION_WIDTHS = (200, 775)
WIDTHS = (1, 63, 64, 65, 127, 129, 200, 775)
N_QUERIES = 65
PAIRED, ALT_ONLY, NO_ALT, EMPTY, SHORT_ALT, N_VARIANTS = 24, 24, 25, 26, 27, 28

# --------------------------------------------------------------------------------------------- the planner, restated
BLOCK, TILE, LOADS = 256, 64, 8


def plan_genotype(n_seqs, wv, n_variants):
    word_blocks, tiles = -(-wv // BLOCK), -(-n_seqs // TILE)
    grid, samples_grid = min(word_blocks * tiles, (1 << 64) - 1), -(-wv // (BLOCK // 64))          # (the grid saturates at 64 bits)
    too_large = grid if grid > 0x7FFFFFFF else samples_grid if samples_grid > 0x7FFFFFFF else 0
    bad = n_variants == 0 or n_variants > MAX_VARIANTS
    too_many = (not bad) and 2 * n_variants * wv * 8 > PLANE_BYTES
    return dict(block=BLOCK, tile=TILE, word_blocks=word_blocks, tiles=tiles, grid=grid, variants_grid=0 if bad else -(-n_variants // (BLOCK // 64)),
                samples_grid=samples_grid, plane_bytes=0 if bad or too_many else 2 * n_variants * wv * 8, too_large=too_large, bad_variants=int(bad),
                too_many_bytes=int(too_many))


# --------------------------------------------------------------------------------------------- the panel and its layouts
def alleles(n, n_variants=None):
    """(allele of query i uint32[n], n_variants): the panel of the module text; with n_variants given, the pairing rule alone over
    that many variants (no special ones: most alleles of a large panel then have no probe)."""
    v_pairs = PAIRED if n_variants is None else n_variants
    out = np.zeros(n, np.uint32)
    for i in range(n):
        c = i % (2 * v_pairs)
        if c < v_pairs:
            out[i] = 2 * c
        else:
            c -= v_pairs
            out[i] = 2 * (c if c % 2 == 0 else (c - 2) % v_pairs) + 1
    if n_variants is not None:
        return out, n_variants
    for q, al in ((5, 2 * ALT_ONLY + 1), (8, 2 * NO_ALT), (11, 2 * SHORT_ALT), (2, 2 * SHORT_ALT + 1)):
        if q < n:
            out[q] = al
    return out, N_VARIANTS


def layout(name, n, n_variants=None):
    """(order int64[n]: the query at every position, allele_of uint32[n] by position, n_variants)"""
    al, nv = alleles(n, n_variants)
    if name == "grouped":
        order = np.argsort(al, kind="stable")
        return order, al[order], nv
    if name == "interleaved":
        return np.arange(n), al.copy(), nv
    if name == "shuffled":
        order = np.random.default_rng(1000 + n).permutation(n)
        a = al[order]
        a[3::7] = NONE
        return order, a, nv
    raise KeyError(name)


def column_mask(p):
    """A selection in the row format that drops the first edge column a probe hits at threshold 1 and has every bit behind num_cols
    set (junk: it is ignored).  Returns (columns uint8[ceil(n_cols / 8)], the dropped column)."""
    hit = hits_of(p, 1.0)
    drop = next(e for e in p.edges if hit[:, e].any())
    bits = np.ones(-(-p.n_cols // 8) * 8, np.uint8)
    bits[drop] = 0
    return np.packbits(bits), drop


# --------------------------------------------------------------------------------------------- the reference
def hits_of(p, thr):
    """bool[n, n_cols]: the hits a search at `thr` reports, from the definition"""
    mk = np.array([T.min_kmers(int(u), thr) for u in p.us], np.int64)
    return (p.counts >= mk[:, None]) & (p.us > 0)[:, None]


def genotype_of(us, hit, order, allele_of, n_variants, columns=None):
    """dict(ref, alt: uint8[n_variants, ceil(n_cols / 8)], variants uint32[n_variants, 4], samples uint32[n_cols, 2], probes
    uint32[n_variants, 2], calls uint8[n_variants, n_cols] -- 0: 0/0, 1: 0/1, 2: 1/1, 3: missing or unselected): the definition,
    line by line"""
    n_cols = hit.shape[1]
    sel = np.ones(n_cols, bool) if columns is None else np.unpackbits(np.asarray(columns, np.uint8))[:n_cols].astype(bool)
    plane = np.zeros((n_variants, 2, n_cols), bool)
    used = np.zeros((n_variants, 2), np.uint32)
    for pos, q in enumerate(order):
        al = int(allele_of[pos])
        if al == NONE or us[q] == 0:
            continue
        plane[al >> 1, al & 1] |= hit[q] & sel
        used[al >> 1, al & 1] += 1
    r, a = plane[:, 0], plane[:, 1]
    variants = np.stack([(r & ~a).sum(axis=1), (r & a).sum(axis=1), (a & ~r).sum(axis=1), (sel[None, :] & ~r & ~a).sum(axis=1)], axis=1).astype(np.uint32)
    samples = np.stack([a.sum(axis=0), (r | a).sum(axis=0)], axis=1).astype(np.uint32)
    calls = np.full((n_variants, n_cols), 3, np.uint8)
    calls[r & ~a], calls[r & a], calls[a & ~r] = 0, 1, 2
    return dict(ref=np.packbits(r, axis=1), alt=np.packbits(a, axis=1), variants=variants, samples=samples, probes=used, calls=calls)


_results = {}


def planted_genotype(p, thr, name, masked=False, sel=None, n_variants=None):
    """the reference of a planted index under a layout (of its first `sel` queries, default all): computed once per process and
    shared; nobody changes it"""
    n = len(p.seqs) if sel is None else sel
    key = (id(p), thr, name, masked, n, n_variants)
    if key not in _results:
        order, al, nv = layout(name, n, n_variants)
        _results[key] = genotype_of(p.us, hits_of(p, thr), order, al, nv, column_mask(p)[0] if masked else None)
        for a in _results[key].values():
            a.setflags(write=False)
    return _results[key]


def width_case(n_cols):
    return T.planted(n_cols, N_QUERIES, seed=65)


def thresholds(p):
    """1.0 (an exact run), a threshold whose min_kmers sits exactly on a count an edge column holds, and 0"""
    if any(0 < int(p.counts[i, e]) < u for i, u in enumerate(p.us) for e in p.edges):
        return (1.0, p.edge_threshold()[0], 0.0)
    return (1.0, 0.5, 0.0)


# --------------------------------------------------------------------------------------------- non-vacuity
def two_tile_word(p, thr, name="interleaved"):
    """(allele, word, position 1, position 2) of a plane word that probes from two different tiles of k_allele_or feed, or None"""
    order, al, _ = layout(name, len(p.seqs))
    hit = hits_of(p, thr)
    wv = -(-p.n_cols // 64)
    seen = {}
    for pos, q in enumerate(order):
        if al[pos] == NONE or p.us[q] == 0:
            continue
        for w in range(wv):
            if hit[q, 64 * w:64 * w + 64].any():
                first = seen.setdefault((int(al[pos]), w), pos)
                if first // TILE != pos // TILE:
                    return int(al[pos]), w, first, pos
    return None


def check_conditions(p):
    """What the width case of one of CONDITION_WIDTHS must hold at every threshold used, from the reference alone."""
    assert len(p.seqs) == N_QUERIES > TILE
    for thr in thresholds(p):
        for name in LAYOUTS:
            g = planted_genotype(p, thr, name)
            at_edges = g["calls"][:, p.edges]
            for state in range(4):
                assert (at_edges == state).any(), ("no edge column holds state", state, thr, name)
            for j, e in enumerate(p.edges):
                assert len(set(at_edges[:, j].tolist())) >= 2, ("an edge column with one state only", e, thr, name)
            assert (g["probes"][:, 1] == 0).any() and g["probes"][NO_ALT, 1] == 0 and g["probes"][SHORT_ALT, 1] == 0
            assert not g["probes"][EMPTY].any() and (g["calls"][EMPTY] == 3).all() and g["variants"][EMPTY, 3] == p.n_cols
            assert (g["variants"].sum(axis=1) == p.n_cols).all()
        g = planted_genotype(p, thr, "grouped")
        assert g["probes"][SHORT_ALT].tolist() == [1, 0] and g["probes"][ALT_ONLY].tolist() == [0, 1] and g["probes"][NO_ALT].tolist() == [1, 0]
        assert two_tile_word(p, thr) is not None, ("no plane word is fed from two tiles", thr)
        # the shuffled layout's NONE entries take probes away: its reference differs from the panel's
        assert not np.array_equal(planted_genotype(p, thr, "shuffled")["probes"], g["probes"])
        # the mask drops a column that is called without it
        columns, drop = column_mask(p)
        m = planted_genotype(p, thr, "grouped", masked=True)
        assert (g["calls"][:, drop] != 3).any() and (m["calls"][:, drop] == 3).all() and not m["samples"][drop].any()
        assert (m["variants"].sum(axis=1) == p.n_cols - 1).all()
    # grouped and interleaved are the same panel: the same reference
    a, b = planted_genotype(p, 1.0, "grouped"), planted_genotype(p, 1.0, "interleaved")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # the edge threshold moves a call
    thr = thresholds(p)[1]
    assert not np.array_equal(planted_genotype(p, thr, "grouped")["calls"], a["calls"])
