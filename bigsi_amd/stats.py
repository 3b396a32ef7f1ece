"""Sample statistics derived from the device's per-column popcounts (bigsi_hip_column_popcounts): how full each sample's Bloom
filter is, and how much of one filter every other sample shares.  Pure functions of count arrays -- no device, no storage -- so
that the arithmetic is pinned on any host; BIGSI.sample_stats / BIGSI.similar_samples feed them."""
import math

STATS_KEYS = ("sample_name", "colour", "bits_set", "fill", "kmer_fpr", "est_kmers")
SIMILAR_KEYS = ("sample_name", "colour", "bits_shared", "jaccard", "containment")


def derive_sample_stats(counts, m, h, names):
    """One dict per named colour, ascending.  counts[c] = X, the bits set in sample c's filter of m bits and h hashes:
    fill = X / m; kmer_fpr = fill ** h, the chance that a k-mer the sample does not hold matches it all the same;
    est_kmers = -(m / h) * log1p(-X / m), the number of distinct k-mers that fills a filter that far (None for a full one).
    names[c] is None for a deleted sample, which is dropped."""
    out = []
    for c, name in enumerate(names):
        if name is None:
            continue
        x = int(counts[c])
        fill = x / m
        out.append({"sample_name": name, "colour": c, "bits_set": x, "fill": fill, "kmer_fpr": fill ** h,
                    "est_kmers": None if x == m else -(m / h) * math.log1p(-x / m)})
    return out


def derive_similar(counts, mask_count, masked_counts, names, leave_out=None, limit=None):
    """One dict per named colour other than `leave_out`, by Jaccard index descending (stable over ascending colour), cut to `limit`.
    With A = mask_count (bits of the query filter), I = masked_counts[c] (bits the sample shares with it) and X = counts[c]:
    jaccard = I / (A + X - I), containment = I / A; 0.0 where the denominator is 0."""
    a = int(mask_count)
    out = []
    for c, name in enumerate(names):
        if name is None or c == leave_out:
            continue
        i, x = int(masked_counts[c]), int(counts[c])
        u = a + x - i
        out.append({"sample_name": name, "colour": c, "bits_shared": i, "jaccard": i / u if u else 0.0, "containment": i / a if a else 0.0})
    out.sort(key=lambda r: -r["jaccard"])          # stable: ties stay in ascending colour
    return out if limit is None else out[:limit]


def to_csv(rows, keys):
    """Header line with the keys, one line per row, None as an empty field."""
    import csv
    import io
    sink = io.StringIO()
    w = csv.writer(sink, lineterminator="\n")
    w.writerow(keys)
    for r in rows:
        w.writerow(["" if r[k] is None else r[k] for k in keys])
    return sink.getvalue()[:-1]
