"""Locus typing, the host parts: from a FASTA scheme of allele records grouped into loci (PubMLST-style names, or a record -> locus
file) to the record order and the two label arrays the device takes (include/bigsi_hip_typing.h), and from the cells and counts it
leaves to calls, sequence types, the record BIGSI.type_samples returns and its JSON / TSV text.  Pure functions of arrays and names:
no device, no storage."""
import io
import json
import os
import re

import numpy as np

from .frontend import read_fasta

NONE = 0xFFFFFFFF                   # BIGSI_TYPING_NONE
MAX_ALLELE = 0xFFFFFFFE             # BIGSI_TYPING_MAX_ALLELE
MAX_LOCI = 1 << 20                  # BIGSI_TYPING_MAX_LOCI
EXACT_SCORE = 0xFFFFFFFF            # the score of a record all of whose k-mers were found
CELL_BYTES = 12                     # device bytes per (locus, column): a 64-bit key and a 32-bit hit count
NOVEL, NO_ST = "novel", "-"


def key_of(c, u, allele):
    """The device's key of a hit, in Python integers: floor(c (2^32 - 1) / u) << 32 | (0xFFFFFFFF - allele)."""
    return (int(c) * EXACT_SCORE // int(u)) << 32 | (0xFFFFFFFF - int(allele))


def _text_or_path(src):
    if isinstance(src, bytes):
        src = src.decode()
    if isinstance(src, str) and "\n" not in src and os.path.exists(src):
        with open(src) as f:
            return f.read()
    return src


def parse_loci_map(src):
    """{record name: locus} from `record<TAB>locus` lines (text, bytes, a path or a dict); empty lines and #-lines are skipped."""
    if isinstance(src, dict):
        return dict(src)
    out = {}
    for n, line in enumerate(_text_or_path(src).splitlines(), 1):
        if not line.strip() or line.startswith("#"):
            continue
        cells = line.rstrip("\r\n").split("\t")
        if len(cells) != 2 or not cells[0] or not cells[1]:
            raise ValueError("loci map line %d: expected record<TAB>locus, got %r" % (n, line))
        if out.get(cells[0], cells[1]) != cells[1]:
            raise ValueError("loci map line %d: record %r is given two loci" % (n, cells[0]))
        out[cells[0]] = cells[1]
    return out


def parse_scheme(fasta, loci_map=None):
    """(loci, names, alleles, records, locus_of uint32, allele_of uint32) from a scheme (FASTA text, bytes or a path).  A record's
    name is its header up to the first whitespace; its locus is loci_map's (parse_loci_map) when that names the record, otherwise the
    name up to its last "_" (PubMLST: adk_12 is allele 12 of adk), and its allele label the rest of the name, or the whole name when
    the locus is no prefix of it.  loci: the locus names in order of first appearance.  The records come back grouped by locus, in
    file order within a locus; allele_of[i] is the record's index in the FILE -- the identity the device breaks ties by, lowest
    first --, so names[j] / alleles[j] are indexed by identity and records[i], locus_of[i], allele_of[i] by position."""
    if isinstance(fasta, bytes):
        fasta = fasta.decode()
    if isinstance(fasta, str) and not fasta.lstrip().startswith(">") and os.path.exists(fasta):
        recs = read_fasta(fasta)
    else:
        recs = read_fasta(io.StringIO(fasta))
    table = parse_loci_map(loci_map) if loci_map is not None else {}
    loci, index, names, alleles, seqs, locus = [], {}, [], [], [], []
    seen = set()
    for header, seq in recs:
        name = header.split()[0] if header.split() else ""
        if name in seen:
            raise ValueError("record %r occurs twice in the scheme" % name)
        seen.add(name)
        if name in table:
            loc = table[name]
        elif "_" in name and name.rsplit("_", 1)[0] and name.rsplit("_", 1)[1]:
            loc = name.rsplit("_", 1)[0]
        else:
            raise ValueError("record %r: no locus -- its name is not locus_allele and the loci map does not hold it" % name)
        if loc not in index:
            index[loc] = len(loci)
            loci.append(loc)
        names.append(name)
        alleles.append(name[len(loc) + 1:] if name.startswith(loc + "_") and len(name) > len(loc) + 1 else name)
        seqs.append(seq)
        locus.append(index[loc])
    if len(names) > MAX_ALLELE:
        raise ValueError("a scheme holds at most %d records" % MAX_ALLELE)
    locus = np.asarray(locus, dtype=np.uint32)
    order = np.argsort(locus, kind="stable")
    return loci, names, alleles, [seqs[i] for i in order], locus[order], order.astype(np.uint32)


def slices(locus_of, n_loci, n_cols, cell_bytes):
    """[(l0, l1, record positions, their locus_of relative to l0)]: the scheme cut by locus so that the cells of a slice's loci
    (ceil(n_cols / 64) x 64 x 12 bytes each) fit cell_bytes -- at least one locus per slice.  A record goes to its locus's slice only;
    NONE records go nowhere."""
    locus_of = np.asarray(locus_of, dtype=np.uint32)
    per_locus = ((int(n_cols) + 63) // 64) * 64 * CELL_BYTES
    step = max(int(cell_bytes) // per_locus, 1)
    out = []
    locus = np.where(locus_of == NONE, np.int64(-1), locus_of.astype(np.int64))
    for l0 in range(0, int(n_loci), step):
        l1 = min(l0 + step, int(n_loci))
        idx = np.flatnonzero((locus >= l0) & (locus < l1))
        out.append((l0, l1, idx, (locus_of[idx] - np.uint32(l0)).astype(np.uint32)))
    return out


def decode(best):
    """(allele int64 -- -1: no call --, score uint32, exact bool) arrays of the shape of `best` (uint64 keys)."""
    best = np.asarray(best, dtype=np.uint64)
    score = (best >> np.uint64(32)).astype(np.uint32)
    allele = np.where(best != 0, np.int64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF)).astype(np.int64), np.int64(-1))
    return allele, score, (best != 0) & (score == np.uint32(EXACT_SCORE))


def calls(best, names, hits=None):
    """Per locus and column None (no record of the locus hit the column) or {"allele": names[identity], "fraction": score /
    (2^32 - 1), "exact": every k-mer found, "n_hits": the locus's records that hit the column (with `hits` given)}:
    out[l][c], from best uint64[n_loci, n_cols]."""
    allele, score, exact = decode(best)
    out = []
    for l in range(allele.shape[0]):
        row = [None] * allele.shape[1]
        for c in np.flatnonzero(allele[l] >= 0):
            rec = {"allele": names[int(allele[l, c])], "fraction": int(score[l, c]) / float(EXACT_SCORE), "exact": bool(exact[l, c])}
            if hits is not None:
                rec["n_hits"] = int(hits[l][c])
            row[c] = rec
        out.append(row)
    return out


def parse_profiles(src, loci):
    """{(allele label of loci[0], of loci[1], ...): ST} from a PubMLST profiles table (text, bytes or a path): a header line
    ST<TAB>locus..., one line per sequence type.  Columns that are no locus of the scheme (clonal_complex, species) are ignored; a
    locus without a column is refused."""
    lines = [x.rstrip("\r\n") for x in _text_or_path(src).splitlines() if x.strip()]
    if not lines:
        raise ValueError("the profiles table is empty")
    header = lines[0].split("\t")
    if header[0] != "ST":
        raise ValueError("the profiles table must start with an ST column, got %r" % header[0])
    missing = [x for x in loci if x not in header[1:]]
    if missing:
        raise ValueError("the profiles table has no column for the loci %s" % ", ".join(missing))
    at = [header.index(x, 1) for x in loci]
    out = {}
    for n, line in enumerate(lines[1:], 2):
        cells = line.split("\t")
        if len(cells) < len(header):
            raise ValueError("profiles line %d has %d columns, the header %d" % (n, len(cells), len(header)))
        out.setdefault(tuple(cells[i] for i in at), cells[0])
    return out


def assign_st(profiles, row):
    """The sequence type of one sample from its calls (one per locus, None: no call): the ST of the row of `profiles`
    (parse_profiles) whose allele labels match when every locus is exact, "novel" when all loci are exact but no row matches, "-"
    otherwise."""
    if any(c is None or not c["exact"] for c in row):
        return NO_ST
    return profiles.get(tuple(c["allele"] for c in row), NOVEL)


def result(loci, locus_counts, sample_counts, records, name_of, excluded=(), call_matrix=None, profiles=None):
    """What BIGSI.type_samples returns.  locus_counts uint32[n_loci, 3], sample_counts uint32[n_cols, 2], records uint32[n_loci];
    call_matrix: calls() over the allele LABELS, or None for a summary (the samples then carry no "calls" and no "ST"); profiles:
    parse_profiles(), or None.  name_of: colour -> name.  Excluded (deleted) colours appear nowhere."""
    locus_counts, sample_counts, records = np.asarray(locus_counts), np.asarray(sample_counts), np.asarray(records)
    ex = set(int(c) for c in np.asarray(excluded).reshape(-1))
    out_loci = [{"name": name, "records": int(records[l]), "called": int(locus_counts[l, 0]), "exact": int(locus_counts[l, 1]),
                 "multiple": int(locus_counts[l, 2])} for l, name in enumerate(loci)]
    samples = []
    for c in range(sample_counts.shape[0]):
        if c in ex:
            continue
        rec = {"sample_name": name_of(c), "colour": c, "called": int(sample_counts[c, 0]), "exact": int(sample_counts[c, 1])}
        if call_matrix is not None:
            row = [call_matrix[l][c] for l in range(len(loci))]
            if profiles is not None:
                rec["ST"] = assign_st(profiles, row)
            rec["calls"] = {name: row[l] for l, name in enumerate(loci) if row[l] is not None}
        samples.append(rec)
    return {"loci": out_loci, "samples": samples}


def to_json(res):
    return json.dumps(res)


def _cell(s):
    return re.sub(r"[\t\r\n]", " ", str(s))


def _call_text(c):
    if c is None:
        return "-"
    return _cell(c["allele"]) if c["exact"] else "%s~%.4f" % (_cell(c["allele"]), c["fraction"])


def to_tsv(res, summary_only=False):
    """The matrix: header sample<TAB>[ST<TAB>]locus..., one line per sample; a cell is the allele label of an exact call,
    label~fraction of a partial one, "-" without a call.  summary_only: per locus its counts, then per sample called / exact."""
    if summary_only:
        lines = ["locus\trecords\tcalled\texact\tmultiple"]
        lines += ["%s\t%d\t%d\t%d\t%d" % (_cell(x["name"]), x["records"], x["called"], x["exact"], x["multiple"]) for x in res["loci"]]
        lines.append("sample\tcolour\tcalled\texact")
        lines += ["%s\t%d\t%d\t%d" % (_cell(s["sample_name"]), s["colour"], s["called"], s["exact"]) for s in res["samples"]]
        return "\n".join(lines)
    loci = [x["name"] for x in res["loci"]]
    with_st = any("ST" in s for s in res["samples"])
    lines = ["sample\t" + ("ST\t" if with_st else "") + "\t".join(_cell(x) for x in loci)]
    for s in res["samples"]:
        head = _cell(s["sample_name"]) + ("\t" + _cell(s.get("ST", NO_ST)) if with_st else "")
        lines.append(head + "\t" + "\t".join(_call_text(s["calls"].get(x)) for x in loci))
    return "\n".join(lines)
