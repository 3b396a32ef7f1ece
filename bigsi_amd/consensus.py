"""How many members of a group must hold a bit for the group's consensus column to keep it (bigsi_hip_consensus_columns_into takes
the answer as one uint32 per group).  Pure functions of integers -- no device, no storage -- so that the rule is pinned on any host;
BIGSI.consensus and HipHbmStorage feed them."""
import numpy as np

NEVER = 0xFFFFFFFF            # the largest threshold there is: no group has that many members, the column is zero


def check_percent(percent):
    """`percent` as the int in [1, 100] it must be: TypeError for anything else than an int (bool and float included), ValueError
    out of range."""
    if isinstance(percent, bool) or not isinstance(percent, (int, np.integer)):
        raise TypeError("percent must be an int in [1, 100], got %r" % (percent,))
    if not 1 <= int(percent) <= 100:
        raise ValueError("percent must be in [1, 100], got %d" % int(percent))
    return int(percent)


def need_of(sizes, percent):
    """uint32[G]: need = max(1, ceil(percent x size / 100)) for every group size, in integers only ((percent x size + 99) // 100), so
    no rounding question arises.  percent=100 is the AND of the members (need = size), percent=1 the OR up to 100 members; a group
    without members needs 1 (and stays zero)."""
    percent = check_percent(percent)
    arr = np.asarray(sizes)
    if arr.ndim != 1 or (arr.size and (arr.dtype.kind not in "ui" or int(arr.min()) < 0 or int(arr.max()) > NEVER)):
        raise ValueError("sizes must be a list of unsigned 32-bit group sizes")
    need = (arr.astype(np.uint64) * np.uint64(percent) + np.uint64(99)) // np.uint64(100)
    return np.maximum(need, np.uint64(1)).astype(np.uint32)


def group_sizes(group_of, num_groups):
    """The number of columns every group of a collapse map has (collapse.DROPPED entries belong to none)."""
    from .collapse import DROPPED
    arr = np.asarray(group_of, dtype=np.uint32)
    return np.bincount(arr[arr != DROPPED].astype(np.int64), minlength=int(num_groups)).astype(np.uint32)


def member_counts(min_members, num_groups):
    """A caller's `min_members` as the contiguous uint32 array the C entry point reads: num_groups entries, unsigned 32-bit, none of
    them 0 (the C call checks that again and names the group)."""
    arr = np.asarray(min_members)
    if arr.ndim != 1 or arr.size != int(num_groups):
        raise ValueError("min_members has %d entries, there are %d groups" % (arr.size, int(num_groups)))
    if arr.size and (arr.dtype.kind not in "ui" or int(arr.min()) < 0 or int(arr.max()) > NEVER):
        raise ValueError("min_members must hold unsigned 32-bit member counts")
    if arr.size and int(arr.min()) == 0:
        raise ValueError("min_members[%d] is 0: a group needs at least one member to keep a bit" % int(np.flatnonzero(arr == 0)[0]))
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return arr if arr.size else np.ones(1, np.uint32)
