"""K-mer prevalence: for every k-mer position of a query, how many samples hold the k-mer (bigsi_hip_kmer_prevalence does the sweep).
The host's share -- which samples count at all (the universe mask), which of them are the named subset, and the records handed back
-- as pure functions of name lists and count arrays: no device, no storage, so that they are pinned on any host.
BIGSI.kmer_prevalence / kmer_prevalence_many and the `prevalence` command feed them."""
import numpy as np

from .graph.metadata import DELETION_SPECIAL_SAMPLE_NAME

RECORD_KEYS = ("num_kmers", "num_unique", "num_samples", "subset_size", "samples_with_kmer", "subset_with_kmer")
CSV_KEYS = ("record", "pos", "kmer", "samples", "in_subset")


def pack_mask(flags):
    """bool per column -> the mask in the row format: ceil(n / 8) bytes, column c at byte c // 8 under 0x80 >> (c % 8); one zero byte
    for an index without columns (a mask is never an empty buffer)."""
    flags = np.asarray(flags, dtype=bool)
    return np.packbits(flags) if flags.size else np.zeros(1, np.uint8)


def universe_mask(num_cols, names):
    """names[c] = the name of colour c, None or DELETION_SPECIAL_SAMPLE_NAME for a deleted sample (BIGSI._sample_names) -> (mask of
    num_cols columns, number of colours in it): every column that has a name.  The matrix may be wider than the metadata (columns
    reserved or written ahead of their records): such columns are in no universe, as `stats` and `similar` leave them out; names at
    or beyond num_cols name no column."""
    flags = np.zeros(int(num_cols), dtype=bool)
    for c, n in enumerate(names[:int(num_cols)]):
        flags[c] = n is not None and n != DELETION_SPECIAL_SAMPLE_NAME
    return pack_mask(flags), int(flags.sum())


def subset_mask(num_cols, names, samples):
    """names as for universe_mask, samples = the names of the subset -> (mask of num_cols columns, number of colours in it).
    ValueError, with the name, for a name that is unknown or deleted (or whose colour the matrix does not hold), for a name given
    twice and for an empty list; TypeError for a bare string."""
    if isinstance(samples, (str, bytes)):
        raise TypeError("samples must be a list of sample names, got %r" % type(samples))
    samples = list(samples)
    if not samples:
        raise ValueError("a subset needs at least one sample")
    colour_of = {n: c for c, n in enumerate(names[:int(num_cols)]) if n is not None and n != DELETION_SPECIAL_SAMPLE_NAME}
    flags = np.zeros(int(num_cols), dtype=bool)
    for s in samples:
        if s == DELETION_SPECIAL_SAMPLE_NAME or s not in colour_of:
            raise ValueError("no sample named %r in the index (unknown or deleted)" % (s,))
        if flags[colour_of[s]]:
            raise ValueError("sample %r is named twice" % (s,))
        flags[colour_of[s]] = True
    return pack_mask(flags), int(flags.sum())


def count_unique(seq, k):
    """Distinct k-mer STRINGS among the windows of seq (a k-mer and its reverse complement are two, as for a search).  A HOST count:
    the definition K1 dedupes by, not the device's num_unique, which the prevalence calls do not return."""
    return len({seq[i:i + k] for i in range(len(seq) - k + 1)})


def assemble(seqs, k, pos_offsets, total, in_subset, num_samples, subset_size):
    """One record per sequence from the flat arrays of the device call: positions [pos_offsets[i], pos_offsets[i + 1]) are sequence
    i's.  in_subset / subset_size None: no subset was asked for."""
    out = []
    for i, s in enumerate(seqs):
        a, b = int(pos_offsets[i]), int(pos_offsets[i + 1])
        n = max(len(s) - k + 1, 0)
        if b - a != n:
            raise ValueError("sequence %d has %d k-mer positions, the device reported %d" % (i, n, b - a))
        out.append({"num_kmers": n, "num_unique": count_unique(s, k), "num_samples": int(num_samples),
                    "subset_size": None if in_subset is None else int(subset_size),
                    "samples_with_kmer": [int(x) for x in total[a:b]],
                    "subset_with_kmer": None if in_subset is None else [int(x) for x in in_subset[a:b]]})
    return out


def to_csv(records, queries, k):
    """record,pos,kmer,samples,in_subset -- one line per k-mer position; `record` is the query's number, kmer the window's text,
    in_subset empty without a subset."""
    import csv
    import io
    sink = io.StringIO()
    w = csv.writer(sink, lineterminator="\n")
    w.writerow(CSV_KEYS)
    for r, (rec, q) in enumerate(zip(records, queries)):
        sub = rec["subset_with_kmer"]
        for p, n in enumerate(rec["samples_with_kmer"]):
            w.writerow([r, p, q[p:p + k], n, "" if sub is None else sub[p]])
    return sink.getvalue()[:-1]
