"""Sample-to-sample distances derived from the device's pairwise popcounts (bigsi_hip_pairwise_popcounts: the bits every pair of
samples' Bloom filters share), and the groups of near-duplicates they make -- the groups `collapse` takes.  Pure functions of count
arrays and name lists -- no device, no storage -- so that the arithmetic is pinned on any host; BIGSI.sample_distances /
BIGSI.cluster_samples feed them."""
import numpy as np

MAX_PAIRS = 1 << 28          # pairs of one device call (BIGSI_PAIRWISE_MAX_PAIRS: 2 GiB of uint64)


def derive_distances(inter, set_a, set_b):
    """inter[i][j] = I, the bits sample i of the first list shares with sample j of the second; set_a[i] = X_i and set_b[j] = X_j,
    the bits of their own filters -> (jaccard, containment), float64 arrays of inter's shape:
    jaccard = I / (X_i + X_j - I), containment = I / X_i (how much of sample i's filter sample j holds); 0.0 where the denominator is
    0.  The arithmetic of stats.derive_similar with sample i as the query -- one correctly rounded division of two integers below
    2^53 -- so that row i here and similar_samples(i) can be compared exactly."""
    inter = np.asarray(inter, dtype=np.uint64)
    xa = np.asarray(set_a, dtype=np.uint64).reshape(-1, 1)
    xb = np.asarray(set_b, dtype=np.uint64).reshape(1, -1)
    if inter.ndim != 2 or inter.shape != (xa.size, xb.size):
        raise ValueError("inter must be a %d x %d matrix" % (xa.size, xb.size))
    i = inter.astype(np.float64)
    union = (xa + xb - inter).astype(np.float64)          # (exact in uint64: I <= min(X_i, X_j))
    own = np.broadcast_to(xa.astype(np.float64), inter.shape)
    jaccard = np.divide(i, union, out=np.zeros(inter.shape, np.float64), where=union != 0)
    containment = np.divide(i, own, out=np.zeros(inter.shape, np.float64), where=own != 0)
    return jaccard, containment


def cluster_single_linkage(jaccard, names, min_jaccard):
    """Single linkage: samples i and j are in one group when a chain of pairs with jaccard >= min_jaccard joins them (a union-find
    over the pairs of the square matrix; either triangle may say so).  names[i] is the name of sample i, the list in colour order.
    Returns an ordered mapping group name -> [member names], the form BIGSI.collapse takes: the groups by their lowest member, a
    group under its lowest member's name, the members in the order of `names`, singletons kept."""
    j = np.asarray(jaccard, dtype=np.float64)
    n = len(names)
    if j.shape != (n, n):
        raise ValueError("jaccard must be a %d x %d matrix" % (n, n))
    if len(set(names)) != n:
        raise ValueError("a sample is named twice")
    if not 0.0 < float(min_jaccard) <= 1.0:
        raise ValueError("min_jaccard must be in (0, 1], got %r" % (min_jaccard,))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(*np.nonzero(j >= float(min_jaccard))):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)          # (the root of a group is its lowest member)
    groups = {}
    for i in range(n):
        groups.setdefault(names[find(i)], []).append(names[i])
    return groups


def to_matrix_csv(matrix, row_names, col_names):
    """A matrix as CSV: a header line with an empty first field and the column names, then one line per row under its name."""
    import csv
    import io
    sink = io.StringIO()
    w = csv.writer(sink, lineterminator="\n")
    w.writerow([""] + list(col_names))
    for name, row in zip(row_names, np.asarray(matrix).tolist()):
        w.writerow([name] + row)
    return sink.getvalue()[:-1]


def groups_to_tsv(groups):
    """A mapping group -> [samples] as the text `collapse --groups FILE` reads: one sample<TAB>group line per member, the groups
    in the mapping's order (a group's colour follows its first appearance)."""
    lines = []
    for g, members in groups.items():
        for s in members:
            if "\t" in s or "\t" in g or "\n" in s or "\n" in g or not s.strip() or not g.strip():
                raise ValueError("the names %r / %r cannot be written as a sample<TAB>group line" % (s, g))
            lines.append("%s\t%s\n" % (s, g))
    return "".join(lines)
