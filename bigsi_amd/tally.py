"""Query-set tally, the host parts: from the two per-sample vectors and the four totals the device leaves (include/bigsi_hip_tally.h)
to the record BIGSI.tally returns and its JSON / CSV text.  Pure functions of arrays and names: no device, no storage."""
import json

import numpy as np

CSV_HEADER = "sample_name,colour,queries_hit,kmers_found"


def order(queries_hit, excluded=()):
    """The colours to report, in report order: every colour with queries_hit > 0 that is not excluded, most queries first, ties to
    the lowest colour."""
    qh = np.asarray(queries_hit, dtype=np.uint64).reshape(-1)
    keep = qh > 0
    ex = np.asarray(excluded, dtype=np.int64).reshape(-1)
    keep[ex[(ex >= 0) & (ex < qh.size)]] = False
    colours = np.flatnonzero(keep)
    # (a stable sort of ascending colours by descending count; uint64 counts are compared as they are, not negated)
    return colours[np.argsort(qh[colours].max(initial=0) - qh[colours], kind="stable")]


def rows(queries_hit, kmers_found, name_of, excluded=(), limit=None):
    """[{"sample_name", "colour", "queries_hit", "kmers_found"}] in report order; limit=N keeps the first N.  name_of: colour -> name."""
    if limit is not None:
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)):
            raise TypeError("limit must be an integer, got %r" % type(limit))
        if limit < 1:
            raise ValueError("limit must be >= 1, got %d" % limit)
    colours = order(queries_hit, excluded)
    if limit is not None:
        colours = colours[:int(limit)]
    return [{"sample_name": name_of(int(c)), "colour": int(c), "queries_hit": int(queries_hit[c]), "kmers_found": int(kmers_found[c])} for c in colours]


def record(queries_hit, kmers_found, totals, name_of, excluded=(), limit=None):
    """What BIGSI.tally returns.  totals: (queries counted, their unique k-mers, queries skipped, counted queries with a hit)."""
    return {"queries": int(totals[0]), "kmers": int(totals[1]), "skipped": int(totals[2]), "queries_with_hits": int(totals[3]),
            "samples": rows(queries_hit, kmers_found, name_of, excluded, limit)}


def to_json(rec):
    return json.dumps(rec)


def to_csv(rec):
    """One line per reported sample under CSV_HEADER; names are quoted the way the search CSV quotes them (a name with a comma, a
    quote or a line break in double quotes, quotes doubled)."""
    def field(s):
        s = str(s)
        return '"%s"' % s.replace('"', '""') if any(ch in s for ch in ',"\r\n') else s
    lines = [CSV_HEADER]
    lines += ["%s,%d,%d,%d" % (field(r["sample_name"]), r["colour"], r["queries_hit"], r["kmers_found"]) for r in rec["samples"]]
    return "\n".join(lines)
