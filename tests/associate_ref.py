"""Support shared by tests/test_associate_host.py and tests/test_gpu_associate.py (a plain module: nothing here is collected): the numpy
reference of the group association (include/bigsi_hip_associate.h) over tally_ref's planted indexes -- `us` and `counts` come from the
finished matrix, never from the plan --, the group layouts the cases use, a hit-dense planted case, a plain Python restatement of the
host planner plan_associate (csrc/bigsi_launch.hpp) that the host test pins against the compiled header, and the conditions the cases
must hold so that a GPU comparison cannot pass emptily.

The layouts: classify_ref's "edges" (eight groups, column 63 in none) and "spread" (seven); "two" -- cases = the even columns (group
0), controls = the odd ones (group 1), column 63 in no group: the shape of a GWAS; "full64" -- 64 groups by c % 64, the higher ones
empty where n_cols < 64: every mask row the kernel can take, eight passes of its group block."""
import numpy as np

import classify_ref as CR
import tally_ref as T
from oracle import coracle
from raw_index import rand_seq

NONE = 0xFFFFFFFF
MAX_GROUPS = 64
INFO_FIELDS = ("num_unique", "min_kmers", "samples_hit", "grouped_hit")
INFO_DTYPE = np.dtype([(f, np.uint32) for f in INFO_FIELDS])
LAYOUTS = ("edges", "spread", "two", "full64")
CONDITION_WIDTHS = (200, 775)

# --------------------------------------------------------------------------------------------- the planner, restated
BLOCK, QUERIES, GROUP_BLOCK = 256, 4, 8


def plan_associate(n_seqs, wv, n_groups):
    bad = n_groups == 0 or n_groups > MAX_GROUPS
    grid, mask_grid = -(-n_seqs // QUERIES), -(-wv // (BLOCK // 64))
    too_large = grid if grid > 0x7FFFFFFF else mask_grid if mask_grid > 0x7FFFFFFF else 0
    return dict(block=BLOCK, grid=grid, mask_grid=mask_grid, lds_bytes=(BLOCK // 64) * QUERIES * (GROUP_BLOCK + 1) * 4,
                passes=0 if bad else -(-n_groups // GROUP_BLOCK), mask_bytes=0 if bad else n_groups * wv * 8, too_large=too_large, bad_groups=int(bad))


# --------------------------------------------------------------------------------------------- the layouts
def layout(name, n_cols):
    """(group_of uint32[n_cols], n_groups)"""
    if name in CR.LAYOUTS:
        return CR.layout(name, n_cols)
    c = np.arange(n_cols)
    if name == "two":
        g = (c % 2).astype(np.uint32)
        g[63:64] = NONE
        return g, 2
    if name == "full64":
        return (c % 64).astype(np.uint32), 64
    raise KeyError(name)


def sizes_of(group_of, n_groups):
    return np.bincount(group_of[group_of != NONE].astype(np.int64), minlength=n_groups).astype(np.int64)


# --------------------------------------------------------------------------------------------- the reference
def group_counts_of(us, counts, thr, group_of, n_groups):
    """(uint32[n, n_groups], INFO_DTYPE[n]): the definition, line by line"""
    out = np.zeros((len(us), n_groups), np.uint32)
    info = np.zeros(len(us), INFO_DTYPE)
    n_cols = counts.shape[1]
    for i, (u, c) in enumerate(zip(us, counts)):
        u = int(u)
        if u == 0:
            continue                                            # all zeros, min_kmers included
        mk = T.min_kmers(u, thr)
        samples = grouped = 0
        for s in range(n_cols):
            if int(c[s]) >= mk:
                samples += 1
                g = int(group_of[s])
                if g != NONE:
                    out[i, g] += 1
                    grouped += 1
        info[i] = (u, mk, samples, grouped)
    return out, info


_results = {}


def planted_counts(p, thr, name):
    """(counts, info) of every query of a planted index under a layout: computed once per process and shared; nobody changes them"""
    key = (id(p), thr, name)
    if key not in _results:
        g, n = layout(name, p.n_cols)
        _results[key] = group_counts_of(p.us, p.counts, thr, g, n)
        for a in _results[key]:
            a.setflags(write=False)
    return _results[key]


def thresholds(p):
    return CR.thresholds(p)


# --------------------------------------------------------------------------------------------- the hit-dense case
DENSE_QUERIES = 9


class Dense(T.Planted):
    """tally_ref.Planted's fields and methods over another pattern: the same 2 % background, and every query i but the zero-hit and
    the short one planted WHOLE into the columns c with (3 c + i) % 7 < 3 -- three columns in seven, in every result word and on both
    sides of every group boundary of the layouts."""

    def __init__(self, n_cols, n_seqs=DENSE_QUERIES, seed=77):
        rng = np.random.default_rng(seed)
        self.n_cols, self.edges = n_cols, T.edge_columns(n_cols)
        lengths = [T.K + int(rng.integers(8, 60)) for _ in range(n_seqs)]
        self.zero_hit, self.short = 1, 2
        lengths[self.short] = 20
        self.seqs = [rand_seq(rng, n) for n in lengths]
        bits = (rng.random((T.M, n_cols), dtype=np.float32) < 0.02).astype(np.uint8)
        rows_of = []
        for s in self.seqs:
            first, _ = coracle.unique_kmers(s, T.K)
            rows_of.append(coracle.seq_rows(s, T.K, T.H, T.M)[first].astype(np.int64))
        cols = np.arange(n_cols)
        for i, rows in enumerate(rows_of):
            if i in (self.zero_hit, self.short):
                continue
            held = cols[(3 * cols + i) % 7 < 3]
            bits[np.ix_(np.unique(rows.ravel()), held)] = 1
        bits[rows_of[self.zero_hit].ravel(), :] = 0
        self.dense = np.packbits(bits, axis=1)
        pairs = [T.counts_of(self.dense, n_cols, T.H, s) for s in self.seqs]
        self.us = np.array([u for u, _ in pairs], np.int64)
        self.counts = np.stack([c for _, c in pairs])
        self.counts.setflags(write=False)


_dense = {}


def dense_case(n_cols):
    """built once per process and shared; nobody changes it"""
    if n_cols not in _dense:
        _dense[n_cols] = Dense(n_cols)
    return _dense[n_cols]


# --------------------------------------------------------------------------------------------- non-vacuity
def check_conditions(p, dense):
    """What the width case `p` and the hit-dense case `dense` of one of CONDITION_WIDTHS must hold, from the reference alone."""
    n_cols = p.n_cols
    assert dense.n_cols == n_cols
    edge_thr = p.edge_threshold()[0]
    # under "two" some record hits part of the cases and part of the controls, and not equally many
    g, n_groups = layout("two", n_cols)
    sizes = sizes_of(g, n_groups)
    assert sizes.sum() == n_cols - 1 and (sizes > 0).all()
    partial = [False]
    for case in (p, dense):
        for thr in (1.0, edge_thr):
            c, _ = planted_counts(case, thr, "two")
            partial.append((((c > 0) & (c < sizes[None, :])).all(axis=1) & (c[:, 0] != c[:, 1])).any())
    assert any(partial), "no record with two partial, different group counts"
    c, _ = planted_counts(dense, 1.0, "two")
    assert (((c > 0) & (c < sizes[None, :])).all(axis=1) & (c[:, 0] != c[:, 1])).any(), "... on the dense case"
    # the dense case is hit-dense
    _, info = planted_counts(dense, 1.0, "two")
    assert (info["samples_hit"].astype(np.int64) * 3 >= n_cols).any(), "no record hits a third of the columns"
    for case in (p, dense):
        for name in LAYOUTS:
            g, n_groups = layout(name, n_cols)
            sizes = sizes_of(g, n_groups)
            # at threshold 0 every column is a hit
            c, info = planted_counts(case, 0.0, name)
            live = case.us > 0
            assert live.any() and (c[live] == sizes[None, :]).all() and (info["samples_hit"][live] == n_cols).all()
            # the zero-hit and the short query
            c1, info1 = planted_counts(case, 1.0, name)
            assert case.us[case.short] == 0 and not c1[case.short].any() and tuple(info1[case.short]) == (0, 0, 0, 0) and not c[case.short].any()
            assert case.us[case.zero_hit] > 0 and info1["samples_hit"][case.zero_hit] == 0 and info1["min_kmers"][case.zero_hit] == case.us[case.zero_hit]
            assert (info1["grouped_hit"] == c1.sum(axis=1)).all()
        # a hit in the ungrouped column
        for name in ("two", "edges"):
            _, info = planted_counts(case, 1.0, name)
            assert (info["samples_hit"] > info["grouped_hit"]).any(), "no hit in an ungrouped column"
    # at the edge threshold some count differs from threshold 1's
    assert any((planted_counts(p, edge_thr, name)[0] != planted_counts(p, 1.0, name)[0]).any() for name in LAYOUTS)
    assert (planted_counts(p, edge_thr, "two")[0] != planted_counts(p, 1.0, "two")[0]).any()
    # full64 has an empty group only where the index is narrower than 64 columns
    assert (sizes_of(*layout("full64", n_cols)) > 0).all() and (sizes_of(*layout("full64", 63)) == 0).sum() == 1
