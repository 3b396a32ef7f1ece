"""Group association, the host parts: from sample groups to the group_of array the device takes (include/bigsi_hip_associate.h), and
from the per-record, per-group sample counts it leaves to 2x2 tables, prevalence, odds ratio, Pearson's chi-square and their TSV /
JSON text.  Pure functions of arrays and names: no device, no storage, no scipy."""
import json
import math

import numpy as np

from .classify import NONE, classify_plan

MAX_GROUPS = 64          # BIGSI_ASSOCIATE_MAX_GROUPS
INFO_FIELDS = ("num_unique", "min_kmers", "samples_hit", "grouped_hit")
INFO_DTYPE = np.dtype([(f, np.uint32) for f in INFO_FIELDS])          # bigsi_hip_associate_info
assert INFO_DTYPE.itemsize == 16

STAT_COLUMNS = ("hit", "prevalence", "log2_odds", "chi2", "p")


def associate_plan(names, groups, others=None):
    """classify.classify_plan(names, groups, others) -- its group_of and group names, and its refusals -- with at most MAX_GROUPS
    groups (ValueError), and `sizes`: the live columns of every group, in id order (deleted and unlisted samples are in no group)."""
    group_of, group_names = classify_plan(names, groups, others)
    if len(group_names) > MAX_GROUPS:
        raise ValueError("%d groups: an association takes at most %d" % (len(group_names), MAX_GROUPS))
    sizes = np.bincount(group_of[group_of != NONE].astype(np.int64), minlength=len(group_names)).astype(np.int64)
    return group_of, group_names, sizes


def tables(counts, info, sizes):
    """Per record and group the 2x2 table of group g against the REST OF THE GROUPED samples, as Python integers (a, b, c, d):
        a = counts[g]     group g, hit          b = n_g - a              group g, not hit
        c = H - a         the rest, hit         d = (T - n_g) - c        the rest, not hit
    with n_g = sizes[g], H = the record's grouped_hit and T = sum(sizes).  Returns one list of n_groups tuples per record."""
    counts = np.asarray(counts)
    info = np.asarray(info, dtype=INFO_DTYPE).reshape(-1)
    sizes = [int(x) for x in sizes]
    counts = counts.reshape(info.size, len(sizes))
    total = sum(sizes)
    out = []
    for row, r in zip(counts, info):
        hit = int(r["grouped_hit"])
        out.append([(int(a), n_g - int(a), hit - int(a), (total - n_g) - (hit - int(a))) for a, n_g in zip(row, sizes)])
    return out


def statistics(table):
    """(prevalence, log2_odds, chi2, p) of one 2x2 table (a, b, c, d):
        prevalence = a / (a + b)                                         (0.0 for a group without members)
        log2_odds  = log2((a + .5)(d + .5) / ((b + .5)(c + .5)))           the Haldane-Anscombe form
        chi2       = T (ad - bc)^2 / (n_g (T - n_g) H (T - H))            Pearson, exact integers and ONE true division; 0.0 when
                                                                          the denominator is 0
        p          = erfc(sqrt(chi2 / 2))                                 exact for one degree of freedom"""
    a, b, c, d = (int(x) for x in table)
    n_g, rest, hit, total = a + b, c + d, a + c, a + b + c + d
    prevalence = a / n_g if n_g else 0.0
    log2_odds = math.log2(((2 * a + 1) * (2 * d + 1)) / ((2 * b + 1) * (2 * c + 1)))
    den = n_g * rest * hit * (total - hit)
    chi2 = (total * (a * d - b * c) ** 2) / den if den else 0.0
    return prevalence, log2_odds, chi2, math.erfc(math.sqrt(chi2 / 2))


def result(counts, info, group_names, sizes, min_af=None):
    """What BIGSI.associate returns: {"groups", "sizes", "total" (T, the grouped live samples), "records": [per kept record
    {"index" (its place in the input), "num_kmers", "min_kmers", "samples_hit", "grouped_hit", "groups": {name: {"hit", "prevalence",
    "log2_odds", "chi2", "p"}}}], "dropped": records left out by min_af}.  min_af=F keeps a record only when H / T lies in
    [F, 1 - F] (H / T one true division, 0.0 when no sample is grouped)."""
    if min_af is not None and not 0.0 <= float(min_af) <= 0.5:
        raise ValueError("min_af must be within 0 .. 0.5, got %r" % (min_af,))
    info = np.asarray(info, dtype=INFO_DTYPE).reshape(-1)
    sizes = [int(x) for x in sizes]
    total = sum(sizes)
    records, dropped = [], 0
    for i, (tabs, r) in enumerate(zip(tables(counts, info, sizes), info)):
        hit = int(r["grouped_hit"])
        if min_af is not None:
            af = hit / total if total else 0.0
            if not float(min_af) <= af <= 1.0 - float(min_af):
                dropped += 1
                continue
        per = {}
        for name, t in zip(group_names, tabs):
            prevalence, log2_odds, chi2, p = statistics(t)
            per[name] = {"hit": t[0], "prevalence": prevalence, "log2_odds": log2_odds, "chi2": chi2, "p": p}
        records.append({"index": i, "num_kmers": int(r["num_unique"]), "min_kmers": int(r["min_kmers"]), "samples_hit": int(r["samples_hit"]),
                        "grouped_hit": hit, "groups": per})
    return {"groups": list(group_names), "sizes": sizes, "total": total, "records": records, "dropped": dropped}


def to_json(res, names=None):
    """The result as JSON; names: the input's record names, a "name" per kept record, first."""
    recs = res["records"] if names is None else [dict({"name": names[r["index"]]}, **r) for r in res["records"]]
    return json.dumps(dict(res, records=recs))


def _field(x):
    return str(x).replace("\t", " ").replace("\n", " ").replace("\r", " ")


def tsv_header(group_names):
    return "\t".join(["name", "num_kmers", "samples_hit"] + ["%s:%s" % (_field(g), c) for g in group_names for c in STAT_COLUMNS])


def to_tsv(res, names):
    """One line per kept record under tsv_header (floats by repr; tabs and line breaks in a name are replaced by spaces), then
    `# dropped<TAB>n`."""
    lines = [tsv_header(res["groups"])]
    for r in res["records"]:
        cells = [_field(names[r["index"]]), str(r["num_kmers"]), str(r["samples_hit"])]
        for g in res["groups"]:
            s = r["groups"][g]
            cells += [str(s["hit"])] + [repr(float(s[c])) for c in STAT_COLUMNS[1:]]
        lines.append("\t".join(cells))
    lines.append("# dropped\t%d" % res["dropped"])
    return "\n".join(lines)
