"""Read classification, the host parts: from sample groups to the group_of array the device takes (include/bigsi_hip_classify.h), and
from the 48-byte records it leaves to verdicts, the summary and their TSV / JSON text.  Pure functions of arrays and names: no device,
no storage."""
import json

import numpy as np

from .collapse import DROPPED, collapse_plan
from .graph.metadata import DELETION_SPECIAL_SAMPLE_NAME

NONE = 0xFFFFFFFF          # BIGSI_CLASSIFY_NONE: a column in no group; the group / colour of an absent place
MAX_GROUPS = 4096          # BIGSI_CLASSIFY_MAX_GROUPS
assert NONE == DROPPED

FIELDS = ("num_unique", "min_kmers", "groups_hit", "samples_hit", "best_group", "best_found", "best_colour", "best_samples_hit",
          "second_group", "second_found", "second_colour", "second_samples_hit")
RECORD_DTYPE = np.dtype([(f, np.uint32) for f in FIELDS])          # bigsi_hip_classify_record
assert RECORD_DTYPE.itemsize == 48

SKIPPED, UNCLASSIFIED, ASSIGNED, AMBIGUOUS = "skipped", "unclassified", "assigned", "ambiguous"
TSV_HEADER = "name\tverdict\tgroup\tbest_found\tnum_kmers\tsecond_group\tsecond_found\tbest_sample"


def classify_plan(names, groups, others=None):
    """names[c] = the name of colour c (DELETION_SPECIAL_SAMPLE_NAME for a deleted sample); groups = what collapse.collapse_plan takes
    (an ordered mapping group name -> [sample names], or (sample, group) pairs: the lines of a sample<TAB>group file) ->
    (group_of: uint32[len(names)], NONE for a column in no group; the group names in id order = order of a group's first appearance).
    Deleted and unlisted samples are in no group; with others="NAME" every unlisted live sample joins ONE extra group of that name,
    after the named ones (none is added when no sample is left for it).  collapse_plan's refusals: KeyError for a sample that is
    unknown or deleted; ValueError for a sample in two groups (or twice in one), a group without members, no groups at all, a group
    called DELETION_SPECIAL_SAMPLE_NAME; also ValueError for `others` naming a group that exists and for more than MAX_GROUPS groups."""
    if others is not None and not isinstance(others, str):
        raise TypeError("others must be a group name, got %r" % (others,))
    group_of, group_names, _ = collapse_plan(names, groups)
    group_of = np.array(group_of, dtype=np.uint32)
    group_names = list(group_names)
    if others is not None:
        if others in group_names:
            raise ValueError("others=%r is the name of a listed group" % (others,))
        if others == DELETION_SPECIAL_SAMPLE_NAME:
            raise ValueError("a group cannot be called %s" % DELETION_SPECIAL_SAMPLE_NAME)
        rest = [c for c, n in enumerate(names) if n != DELETION_SPECIAL_SAMPLE_NAME and group_of[c] == NONE]
        if rest:
            group_of[rest] = len(group_names)
            group_names.append(others)
    if len(group_names) > MAX_GROUPS:
        raise ValueError("%d groups: a classification takes at most %d" % (len(group_names), MAX_GROUPS))
    return group_of, group_names


def verdicts(records, group_names, margin=1):
    """One (verdict, group name or None) per record.  The rule:
        num_unique == 0                                          skipped       (the sequence is shorter than k)
        groups_hit == 0                                          unclassified
        groups_hit == 1, or best_found - second_found >= margin  assigned to best_group
        otherwise                                                ambiguous
    At threshold 1.0 every hit found all of a read's k-mers, so a read that two groups hold whole has best_found == second_found and
    is ambiguous at any margin >= 1 -- which is the right answer: nothing in the index tells the two groups apart for this read."""
    if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)):
        raise TypeError("margin must be an integer, got %r" % type(margin))
    if margin < 0:
        raise ValueError("margin must be >= 0, got %d" % margin)
    out = []
    for r in np.asarray(records, dtype=RECORD_DTYPE).reshape(-1):
        if int(r["num_unique"]) == 0:
            out.append((SKIPPED, None))
        elif int(r["groups_hit"]) == 0:
            out.append((UNCLASSIFIED, None))
        elif int(r["groups_hit"]) == 1 or int(r["best_found"]) - int(r["second_found"]) >= margin:
            out.append((ASSIGNED, group_names[int(r["best_group"])]))
        else:
            out.append((AMBIGUOUS, None))
    return out


def rows(records, group_names, name_of, margin=1):
    """One dict per record: verdict, group (the assigned group's name or None), best_sample (the name of best_colour; None when there
    is none or the metadata has no record of the colour), and the record's numbers with group ids replaced by names."""
    def group(g):
        return None if int(g) == NONE else group_names[int(g)]

    def colour(c):
        return None if int(c) == NONE else int(c)
    out = []
    records = np.asarray(records, dtype=RECORD_DTYPE).reshape(-1)
    for r, (verdict, name) in zip(records, verdicts(records, group_names, margin)):
        out.append({"verdict": verdict, "group": name, "best_sample": None if int(r["best_colour"]) == NONE else name_of(int(r["best_colour"])),
                    "num_kmers": int(r["num_unique"]), "min_kmers": int(r["min_kmers"]), "groups_hit": int(r["groups_hit"]), "samples_hit": int(r["samples_hit"]),
                    "best_group": group(r["best_group"]), "best_found": int(r["best_found"]), "best_colour": colour(r["best_colour"]),
                    "best_samples_hit": int(r["best_samples_hit"]), "second_group": group(r["second_group"]), "second_found": int(r["second_found"]),
                    "second_colour": colour(r["second_colour"]), "second_samples_hit": int(r["second_samples_hit"])})
    return out


def summary(rows_, group_names):
    """{"reads", "assigned": {group: reads} (every group, in id order), "ambiguous", "unclassified", "skipped"} of rows()'s dicts."""
    per = {g: 0 for g in group_names}
    counts = {AMBIGUOUS: 0, UNCLASSIFIED: 0, SKIPPED: 0}
    for r in rows_:
        if r["verdict"] == ASSIGNED:
            per[r["group"]] += 1
        else:
            counts[r["verdict"]] += 1
    return {"reads": len(rows_), "assigned": per, "ambiguous": counts[AMBIGUOUS], "unclassified": counts[UNCLASSIFIED], "skipped": counts[SKIPPED]}


def result(records, group_names, name_of, margin=1):
    """What BIGSI.classify returns."""
    rs = rows(records, group_names, name_of, margin)
    return {"groups": list(group_names), "records": rs, "summary": summary(rs, group_names)}


def to_json(res, names=None, summary_only=False):
    """The result as JSON; names: a "name" per record, first.  summary_only leaves the records out."""
    if summary_only:
        return json.dumps({"groups": res["groups"], "summary": res["summary"]})
    recs = res["records"] if names is None else [dict({"name": n}, **r) for n, r in zip(names, res["records"])]
    return json.dumps({"groups": res["groups"], "records": recs, "summary": res["summary"]})


def to_tsv(res, names, summary_only=False):
    """One line per record under TSV_HEADER (an empty field for what a record does not have), then -- or, summary_only, only -- the
    summary as `# key<TAB>value` lines.  Tabs and line breaks in a name are replaced by spaces."""
    def field(x):
        return "" if x is None else str(x).replace("\t", " ").replace("\n", " ").replace("\r", " ")
    lines = []
    if not summary_only:
        lines.append(TSV_HEADER)
        for n, r in zip(names, res["records"]):
            lines.append("\t".join(field(x) for x in (n, r["verdict"], r["group"], r["best_found"], r["num_kmers"], r["second_group"], r["second_found"], r["best_sample"])))
    s = res["summary"]
    lines.append("# reads\t%d" % s["reads"])
    lines += ["# assigned %s\t%d" % (field(g), n) for g, n in s["assigned"].items()]
    lines += ["# %s\t%d" % (key, s[key]) for key in (AMBIGUOUS, UNCLASSIFIED, SKIPPED)]
    return "\n".join(lines)
