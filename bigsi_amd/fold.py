"""Folding an index to a smaller Bloom filter size (bigsi_hip_fold_rows / bigsi_hip_fold_rows_into): which factors exist, and what a
fold is expected to cost in false positives.  Pure functions of integers and count arrays -- no device, no storage -- so that the
arithmetic is pinned on any host; BIGSI.fold / BIGSI.fold_into and the `fold` command feed them.

A row id is floor_mod(signed murmur3(kmer, seed), m) (the reference's bloom/bloomfilter.py:5-6).  For a divisor d of m and
m' = m / d, floor_mod(x, m) mod m' == floor_mod(x, m'): ORing the d rows r, r + m', ..., r + (d - 1) m' into row r gives, bit for
bit, the matrix the same samples build under m'."""

FOLD_KEYS = ("sample_name", "colour", "bits_set", "fill", "est_fill", "est_kmer_fpr")


def fold_plan(m, factor):
    """m' = m / factor for a valid fold.  TypeError for anything but plain ints (a bool is not a factor), ValueError for a factor
    < 1 or one that does not divide m (both numbers in the message)."""
    for what, v in (("m", m), ("factor", factor)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError("%s must be an int, got %r" % (what, v))
    if m < 1:
        raise ValueError("m must be positive, got %d" % m)
    if factor < 1 or m % factor:
        raise ValueError("fold factor %d does not divide num_rows %d" % (factor, m))
    return m // factor


def divisors(m):
    """Every divisor of m, ascending (trial division up to sqrt(m): 5000 steps for a 25 M-row index)."""
    if isinstance(m, bool) or not isinstance(m, int) or m < 1:
        raise ValueError("m must be a positive int, got %r" % (m,))
    small, large = [], []
    d = 1
    while d * d <= m:
        if m % d == 0:
            small.append(d)
            if d != m // d:
                large.append(m // d)
        d += 1
    return small + large[::-1]


def divisors_near(m, target_rows, count=5):
    """The valid fold factors of m (every divisor but 1) whose folded size m / factor lies closest to `target_rows`, at most `count`
    of them, as [(factor, m')] by ascending factor.  [] when m has none (m == 1); a prime m has exactly one, (m, 1)."""
    if isinstance(target_rows, bool) or not isinstance(target_rows, int) or target_rows < 1:
        raise ValueError("target_rows must be a positive int, got %r" % (target_rows,))
    cands = [(d, m // d) for d in divisors(m) if d > 1]
    cands.sort(key=lambda fm: (abs(fm[1] - target_rows), fm[0]))
    return sorted(cands[:max(int(count), 0)])


def fold_estimate(bits_set, m, h, factor):
    """PREDICTED fill and k-mer false-positive rate of every sample after a fold by `factor` -- an estimate, not a measurement: the
    balls-in-bins model stats.derive_sample_stats uses for est_kmers.  A filter with X of m bits set, its bits taken as independent,
    leaves a folded bit clear only if all `factor` bits that feed it are clear: est_fill = 1 - (1 - X / m) ** factor, and
    est_kmer_fpr = est_fill ** h.  The exact figures are sample_stats() of the folded index.  Returns one (est_fill, est_kmer_fpr)
    pair per entry of bits_set."""
    fold_plan(m, factor)
    if isinstance(h, bool) or not isinstance(h, int) or h < 1:
        raise ValueError("h must be a positive int, got %r" % (h,))
    out = []
    for x in bits_set:
        x = int(x)
        if not 0 <= x <= m:
            raise ValueError("a filter of %d bits cannot have %d set" % (m, x))
        fill = 1.0 - (1.0 - x / m) ** factor
        out.append((fill, fill ** h))
    return out


def fold_estimate_rows(stats_rows, m, h, factor):
    """The `fold --dry-run` table: sample_stats() rows (sample_name, colour, bits_set, fill) with est_fill / est_kmer_fpr added."""
    est = fold_estimate([r["bits_set"] for r in stats_rows], m, h, factor)
    return [{"sample_name": r["sample_name"], "colour": r["colour"], "bits_set": r["bits_set"], "fill": r["fill"], "est_fill": f, "est_kmer_fpr": p}
            for r, (f, p) in zip(stats_rows, est)]
