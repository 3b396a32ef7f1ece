"""Which group every column of a collapse goes to (bigsi_hip_collapse_columns_into takes the answer as one uint32 per source column).
Pure functions of name lists -- no device, no storage -- so that the derivation is pinned on any host; BIGSI.collapse and
HipHbmStorage feed them."""
import numpy as np

from .graph.metadata import DELETION_SPECIAL_SAMPLE_NAME

DROPPED = 0xFFFFFFFF          # group_of[c] of a column that goes nowhere (BIGSI_COLLAPSE_DROPPED)


def group_pairs(groups):
    """`groups` as (sample, group) pairs in the order given: an ordered mapping group name -> [sample names], or the pairs themselves.
    Also returns the group names in order of first appearance (a mapping may name a group without members: it is kept, so that the
    plan can refuse it)."""
    if isinstance(groups, (str, bytes)):
        raise TypeError("groups must be a mapping group -> [samples] or (sample, group) pairs, got %r" % type(groups))
    pairs, order = [], []
    if hasattr(groups, "items"):
        for g, members in groups.items():
            if isinstance(members, (str, bytes)):
                raise TypeError("the members of group %r must be a list of sample names, got %r" % (g, type(members)))
            order.append(g)
            pairs.extend((s, g) for s in members)
    else:
        for item in groups:
            s, g = item
            if g not in order:
                order.append(g)
            pairs.append((s, g))
    return pairs, order


def check_groups(groups, keep_others=False):
    """Everything about `groups` that can be refused without the index's names (BIGSI.collapse does so before it touches anything):
    returns group_pairs(groups).  TypeError / ValueError as collapse_plan says."""
    if not isinstance(keep_others, bool):
        raise TypeError("keep_others must be a bool, got %r" % (keep_others,))
    pairs, order = group_pairs(groups)
    if not order:
        raise ValueError("collapse needs at least one group")
    if DELETION_SPECIAL_SAMPLE_NAME in order:
        raise ValueError("a group cannot be called %s" % DELETION_SPECIAL_SAMPLE_NAME)
    first = {}
    for s, g in pairs:
        if s in first:
            raise ValueError("sample %r is in two groups (%r and %r)" % (s, first[s], g) if first[s] != g else "sample %r is named twice in group %r" % (s, g))
        first[s] = g
    empty = [g for g in order if g not in set(first.values())]
    if empty:
        raise ValueError("group %r has no members" % (empty[0],))
    return pairs, order


def collapse_plan(names, groups, keep_others=False):
    """names[c] = the name of colour c (DELETION_SPECIAL_SAMPLE_NAME for a deleted sample); groups = an ordered mapping group name ->
    [sample names], or (sample, group) pairs -> (group_of: uint32[len(names)], DROPPED for a column that goes nowhere; the group names
    in destination colour order = order of a group's first appearance; members per group: sample names in colour order).
    Deleted samples are always dropped.  Unlisted samples are dropped, or with keep_others each becomes a group of its own under its
    own name, after the named groups, in colour order.  KeyError for a sample that is unknown or deleted; ValueError for a sample in
    two groups (or twice in one), a group without members, no groups at all, a group called DELETION_SPECIAL_SAMPLE_NAME and, with
    keep_others, a group name that a kept sample already has."""
    pairs, order = check_groups(groups, keep_others)
    colour_of = {n: c for c, n in enumerate(names) if n != DELETION_SPECIAL_SAMPLE_NAME}
    id_of = {g: i for i, g in enumerate(order)}
    group_of = np.full(len(names), DROPPED, dtype=np.uint32)
    for s, g in pairs:
        if s == DELETION_SPECIAL_SAMPLE_NAME or s not in colour_of:
            raise KeyError(s)
        c = colour_of[s]
        group_of[c] = id_of[g]
    out_names = list(order)
    if keep_others:
        for c, n in enumerate(names):
            if n == DELETION_SPECIAL_SAMPLE_NAME or group_of[c] != DROPPED:
                continue
            if n in id_of:
                raise ValueError("group %r has the name of a sample that is kept on its own" % (n,))
            group_of[c] = len(out_names)
            out_names.append(n)
    members = [[] for _ in out_names]
    for c in np.flatnonzero(group_of != DROPPED).tolist():
        members[int(group_of[c])].append(names[c])
    return group_of, out_names, members


def group_ids(group_of, num_cols, num_groups):
    """A caller's `group_of` as the contiguous uint32 array the C entry point reads: num_cols entries, each below num_groups or
    DROPPED (the C call checks the values again and names the column)."""
    arr = np.asarray(group_of)
    if arr.ndim != 1 or arr.size != num_cols:
        raise ValueError("group_of has %d entries, the index has %d columns" % (arr.size, num_cols))
    if arr.size and (arr.dtype.kind not in "ui" or int(arr.min()) < 0 or int(arr.max()) > DROPPED):
        raise ValueError("group_of must hold unsigned 32-bit group ids")
    if not 0 < int(num_groups) < DROPPED:
        raise ValueError("num_groups %d is not in [1, 2^32 - 1)" % int(num_groups))
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return arr if arr.size else np.zeros(1, np.uint32)
