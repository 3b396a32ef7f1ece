"""Windowed search, the host parts: from the hit lists and records the device (or the CPU twin) leaves (include/bigsi_hip_window.h) to
the dicts BIGSI.search_windows_many returns and their JSON / CSV text.  Pure functions of arrays and names: no device, no storage."""
import csv
import io
import json
import math

import numpy as np

WINDOW_MAX = 65535          # BIGSI_WINDOW_MAX
RECORD_DTYPE = np.dtype([("best_found", np.uint32), ("best_start", np.uint32), ("first_start", np.uint32), ("last_start", np.uint32),
                         ("windows_passing", np.uint32), ("reserved", np.uint32)])          # bigsi_hip_window_hit
RESULT_KEYS = ("sample_name", "colour", "best_found", "percent_found", "best_start", "match_start", "match_end", "windows_passing")
CSV_KEYS = ("record",) + RESULT_KEYS


def check_args(window, threshold):
    """The refusals of the C ABI, as ValueErrors before any device call.  Returns (window, threshold) as int and float."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)):
        raise TypeError("window must be an integer, got %r" % type(window))
    if not 1 <= window <= WINDOW_MAX:
        raise ValueError("window must be 1 .. %d k-mer positions, got %d" % (WINDOW_MAX, window))
    threshold = float(threshold)
    if not 0 < threshold <= 1:
        raise ValueError("threshold must be in (0, 1], got %r" % (threshold,))
    return int(window), threshold


def window_need(n, window, threshold):
    """(We, need) of a sequence with n k-mer positions: We = min(window, n), need = ceil(We * threshold)."""
    we = min(int(window), int(n))
    return we, int(math.ceil(we * threshold))


def assemble(seqs, k, window, threshold, window_used, need, hit_offsets, colours, records, name_of, excluded=()):
    """One dict per sequence: {"num_kmers", "window", "min_found", "results": [...]}; a result is a dict of RESULT_KEYS.  match_start /
    match_end: 0-based base coordinates on the query, [first_start, last_start + We + k - 1).  Results by best_found descending, ties
    to the lowest colour; excluded colours (deleted samples) dropped.  The device's window_used / need must be what window_need says."""
    records = np.asarray(records).view(RECORD_DTYPE).reshape(-1) if np.asarray(records).dtype != RECORD_DTYPE else np.asarray(records)
    ex = set(int(c) for c in np.asarray(excluded).reshape(-1))
    out = []
    for i, s in enumerate(seqs):
        n = max(len(s) - k + 1, 0)
        we, mf = window_need(n, window, threshold)
        if int(window_used[i]) != we or int(need[i]) != mf:
            raise ValueError("sequence %d: the device used a window of %d and needs %d, the host expects %d and %d" % (i, int(window_used[i]), int(need[i]), we, mf))
        lo, hi = int(hit_offsets[i]), int(hit_offsets[i + 1])
        results = []
        for j in sorted((j for j in range(lo, hi) if int(colours[j]) not in ex), key=lambda j: (-int(records[j]["best_found"]), int(colours[j]))):
            r = records[j]
            results.append({"sample_name": name_of(int(colours[j])), "colour": int(colours[j]), "best_found": int(r["best_found"]),
                            "percent_found": 100.0 * int(r["best_found"]) / we, "best_start": int(r["best_start"]),
                            "match_start": int(r["first_start"]), "match_end": int(r["last_start"]) + we + k - 1,
                            "windows_passing": int(r["windows_passing"])})
        out.append({"num_kmers": n, "window": we, "min_found": mf, "results": results})
    return out


def to_json(recs, queries):
    return json.dumps([dict([("query", q)] + list(r.items())) for q, r in zip(queries, recs)])


def to_csv(recs):
    """record,<RESULT_KEYS> with one line per result; `record` is the query's number."""
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator="\n")
    w.writerow(CSV_KEYS)
    for i, rec in enumerate(recs):
        for r in rec["results"]:
            w.writerow([i] + [r[key] for key in RESULT_KEYS])
    return buf.getvalue().rstrip("\n")
