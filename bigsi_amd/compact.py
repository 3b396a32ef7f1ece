"""Which columns a vacuum or an extraction keeps (bigsi_hip_compact_columns / bigsi_hip_extract_columns take the answer as a keep
bitmap).  Pure functions of name lists -- no device, no storage -- so that the derivation is pinned on any host; BIGSI.vacuum /
BIGSI.extract and HipHbmStorage feed them."""
import numpy as np

from .graph.metadata import DELETION_SPECIAL_SAMPLE_NAME


def pack_keep(flags):
    """bool per column -> the keep bitmap in the row format: ceil(n / 8) bytes, column c at byte c // 8 under 0x80 >> (c % 8)."""
    return np.packbits(np.asarray(flags, dtype=bool))


def keep_bytes(keep, num_cols):
    """A caller's `keep` as the uint8 bitmap the C entry points read: a bool array (one entry per column), or the packed bitmap
    itself as a uint8 array / bytes of ceil(num_cols / 8) bytes."""
    nb = (int(num_cols) + 7) // 8
    if isinstance(keep, np.ndarray) and keep.dtype == np.bool_:
        if keep.ndim != 1 or keep.size != num_cols:
            raise ValueError("the keep array has %d entries, the index has %d columns" % (keep.size, num_cols))
        buf = pack_keep(keep)
    elif isinstance(keep, np.ndarray):
        if keep.dtype != np.uint8:
            raise ValueError("a keep array must be bool or uint8, got %s" % keep.dtype)
        buf = np.ascontiguousarray(keep).reshape(-1)
    elif isinstance(keep, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(bytes(keep), dtype=np.uint8)
    else:
        raise TypeError("expected a bool / uint8 array or bytes, got %r" % type(keep))
    if buf.size != nb:
        raise ValueError("the keep bitmap has %d bytes, an index of %d columns takes %d" % (buf.size, num_cols, nb))
    return np.ascontiguousarray(buf) if nb else np.zeros(1, np.uint8)


def vacuum_plan(names):
    """names[c] = the name of colour c (DELETION_SPECIAL_SAMPLE_NAME for a deleted sample) -> (keep bitmap, names of the kept
    colours in their old order: the j-th of them becomes colour j)."""
    flags = [n != DELETION_SPECIAL_SAMPLE_NAME for n in names]
    return pack_keep(flags), [n for n, f in zip(names, flags) if f]


def extract_plan(names, samples):
    """names as for vacuum_plan, samples = the names to extract -> (keep bitmap, the extracted names in COLOUR order, whatever
    order they were asked for in).  ValueError for an empty or repeating list, KeyError for a name that is unknown or deleted."""
    samples = list(samples)
    if not samples:
        raise ValueError("extract needs at least one sample")
    if len(set(samples)) != len(samples):
        seen = set()
        raise ValueError("sample %r is named twice" % next(s for s in samples if s in seen or seen.add(s)))
    colour_of = {n: c for c, n in enumerate(names) if n != DELETION_SPECIAL_SAMPLE_NAME}
    for s in samples:
        if s == DELETION_SPECIAL_SAMPLE_NAME or s not in colour_of:
            raise KeyError(s)
    flags = np.zeros(len(names), dtype=bool)
    flags[[colour_of[s] for s in samples]] = True
    return pack_keep(flags), [names[c] for c in np.flatnonzero(flags).tolist()]
