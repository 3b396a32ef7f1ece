"""Support shared by tests/test_classify_host.py and tests/test_gpu_classify.py (a plain module: nothing here is collected): the numpy
reference of the read classification (include/bigsi_hip_classify.h) over tally_ref's planted indexes -- `us` and `counts` come from the
finished matrix, never from the plan --, the group layouts the cases use, a plain Python restatement of the host planner
plan_classify (csrc/bigsi_launch.hpp) that the host test pins against the compiled header, and the conditions a case must hold so that
a GPU comparison cannot pass emptily.

The layouts, over tally_ref's edge columns e_0 .. e_4 = column 0, 63, 64, the first column of the last result word, the last column
(roles (i + j) % 3 per query i: e_0 and e_3 share a role, e_1 and e_4 share one):
  "edges"   e_0 and e_3 in ONE group (id 0): every third query both hold the full count, in different result words -- the lowest colour
            must win; column 63 in NO group; columns 60-62 and 64-70 group 1, which straddles the first word boundary; the last column
            alone in group 7; every other column in groups 2 .. 6 in blocks of 16 (neighbouring colours share a group, as the samples
            of a species do).  Eight groups.
  "spread"  every edge column a group of its own (0 .. 4), so that e_0 / e_3 and e_1 / e_4 TIE on found and the lower id must win;
            every other column in group 5 or 6 by parity (neighbouring lanes hit different table entries).  Seven groups."""
import numpy as np

import tally_ref as T

NONE = 0xFFFFFFFF
MAX_GROUPS = 4096
FIELDS = ("num_unique", "min_kmers", "groups_hit", "samples_hit", "best_group", "best_found", "best_colour", "best_samples_hit",
          "second_group", "second_found", "second_colour", "second_samples_hit")
DTYPE = np.dtype([(f, np.uint32) for f in FIELDS])
EMPTY = (0, 0, 0, 0, NONE, 0, NONE, 0, NONE, 0, NONE, 0)
LAYOUTS = ("edges", "spread")
CONDITION_WIDTHS = (200, 775)

# --------------------------------------------------------------------------------------------- the planner, restated
BLOCK = 256


def plan_classify(n_seqs, wv, n_groups):
    bad = n_groups == 0 or n_groups > MAX_GROUPS
    table = 0 if bad else -(-n_groups * 12 // 16) * 16
    return dict(block=BLOCK, grid=n_seqs, table_bytes=table, lds_bytes=0 if bad else table + (BLOCK // 64) * 3 * 8,
                too_large=n_seqs if n_seqs > 0x7FFFFFFF else 0, bad_groups=int(bad))


def bad_column(group_of, n_groups):
    bad = np.flatnonzero((group_of != NONE) & (group_of >= n_groups))
    return int(bad[0]) if bad.size else len(group_of)


# --------------------------------------------------------------------------------------------- the layouts
def layout(name, n_cols):
    """(group_of uint32[n_cols], n_groups)"""
    wv = -(-n_cols // 64)
    c = np.arange(n_cols)
    if name == "edges":
        g = ((c // 16) % 5 + 2).astype(np.uint32)
        g[60:71] = 1
        g[[x for x in (0, 64 * (wv - 1)) if x < n_cols]] = 0
        g[63:64] = NONE
        g[n_cols - 1] = 7
        return g, 8
    if name == "spread":
        g = (5 + c % 2).astype(np.uint32)
        for j, e in enumerate((0, 63, 64, 64 * (wv - 1), n_cols - 1)):
            if 0 <= e < n_cols:
                g[e] = j
        return g, 7
    raise KeyError(name)


# --------------------------------------------------------------------------------------------- the reference
def records_of(us, counts, thr, group_of, n_groups):
    """DTYPE[n]: the definition, line by line"""
    out = np.zeros(len(us), DTYPE)
    n_cols = counts.shape[1]
    for i, (u, c) in enumerate(zip(us, counts)):
        u = int(u)
        if u == 0:
            out[i] = EMPTY
            continue
        mk = T.min_kmers(u, thr)
        samples, found, colour = [0] * n_groups, [0] * n_groups, [NONE] * n_groups
        for s in range(n_cols):
            g = int(group_of[s])
            if int(c[s]) >= mk and g != NONE:
                if samples[g] == 0 or int(c[s]) > found[g]:          # the LOWEST hit colour that holds the maximum
                    found[g], colour[g] = int(c[s]), s
                samples[g] += 1
        hit = sorted((g for g in range(n_groups) if samples[g] > 0), key=lambda g: (-found[g], g))
        places = [(g, found[g], colour[g], samples[g]) for g in hit[:2]] + [(NONE, 0, NONE, 0)] * 2
        out[i] = (u, mk, len(hit), sum(samples)) + places[0] + places[1]
    return out


_records = {}


def planted_records(p, thr, name):
    """records of every query of a planted index under a layout: computed once per process and shared; nobody changes them"""
    key = (id(p), thr, name)
    if key not in _records:
        g, n = layout(name, p.n_cols)
        _records[key] = records_of(p.us, p.counts, thr, g, n)
        _records[key].setflags(write=False)
    return _records[key]


def thresholds(p):
    return (1.0, p.edge_threshold()[0], 0.0)


def empty_records(n):
    out = np.zeros(n, DTYPE)
    out[:] = EMPTY
    return out


# --------------------------------------------------------------------------------------------- non-vacuity
def check_conditions(p):
    """What the planted index `p` (one of CONDITION_WIDTHS wide) must hold over the three thresholds and the two layouts the GPU cases
    run, so that none of their comparisons passes emptily: conditions (a) .. (h) of the feature's test plan.  Returns which (layout,
    threshold) pairs meet each, for the caller to look at."""
    met = {x: [] for x in "abcdefgh"}
    n_cols, wv = p.n_cols, -(-p.n_cols // 64)
    for name in LAYOUTS:
        g, n_groups = layout(name, n_cols)
        for thr in thresholds(p):
            rec = planted_records(p, thr, name)
            mk = np.array([T.min_kmers(int(u), thr) for u in p.us], np.int64)
            hit = (p.counts >= mk[:, None]) & (p.us > 0)[:, None]
            where = (name, thr)
            if ((rec["groups_hit"] >= 2) & (rec["best_found"] > rec["second_found"])).any():
                met["a"].append(where)
            tie = (rec["groups_hit"] >= 2) & (rec["best_found"] == rec["second_found"])
            if tie.any():
                assert (rec["best_group"][tie] < rec["second_group"][tie]).all()
                if thr > 0 and (rec["best_found"][tie] > 0).any():
                    met["b"].append(where)
            for i in np.flatnonzero(rec["groups_hit"] >= 1):
                cols = np.flatnonzero(hit[i] & (g == rec["best_group"][i]) & (p.counts[i] == rec["best_found"][i]))
                if thr > 0 and len(set(cols // 64)) >= 2:
                    assert rec["best_colour"][i] == cols[0]
                    met["c"].append(where)
                    break
            if thr > 0 and hit[:, g == NONE].any():
                met["d"].append(where)
            if ((rec["groups_hit"] >= 1) & (rec["groups_hit"] < n_groups)).any():
                met["e"].append(where)
            if thr == 0.0:
                per_group_max = np.stack([np.where(g == x, p.counts, -1).max(axis=1) for x in range(n_groups)], axis=1)
                assert (rec["groups_hit"][p.us > 0] == n_groups).all()          # at threshold 0 every grouped column is a hit
                if (per_group_max[p.us > 0] == 0).any():
                    met["f"].append(where)
            if p.us[p.short] == 0 and tuple(rec[p.short]) == EMPTY and p.us[p.zero_hit] > 0 and (thr == 0.0 or rec["groups_hit"][p.zero_hit] == 0):
                met["g"].append(where)
        members = [np.flatnonzero(g == x) for x in range(n_groups)]
        if any(len(m) >= 2 and m[0] // 64 != m[-1] // 64 and m[0] // 64 == 0 and m[-1] - m[0] < 64 for m in members) and \
                any(m.tolist() == [n_cols - 1] for m in members):
            met["h"].append((name, None))
    assert wv >= 4
    for x, where in met.items():
        assert where, "condition (%s) is met by no (layout, threshold) of the %d-column case" % (x, n_cols)
    # what the layouts were built for
    assert any(name == "edges" for name, _ in met["c"]) and any(name == "edges" for name, _ in met["d"]) and any(name == "spread" for name, _ in met["b"])
    assert any(thr == 1.0 for _, thr in met["b"]) and any(thr == 1.0 for _, thr in met["c"])
    return met
