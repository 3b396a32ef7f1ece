"""Panel genotyping, the host parts: from a FASTA panel of variant probes to the probe order and allele_of the device takes
(include/bigsi_hip_genotype.h), and from the two bit planes and the counts it leaves to calls, the record BIGSI.genotype_panel returns
and its JSON / TSV text.  Pure functions of arrays and names: no device, no storage."""
import io
import json
import os
import re

import numpy as np

from .frontend import read_fasta

NONE = 0xFFFFFFFF                   # BIGSI_GENOTYPE_NONE
MAX_VARIANTS = 1 << 20              # BIGSI_GENOTYPE_MAX_VARIANTS
GENOTYPES = ("0/0", "0/1", "1/1", "./.")          # the order of variant_counts: hom_ref, het, hom_alt, missing


def parse_panel(fasta):
    """(variant names, probes ordered by allele, allele_of uint32[len(probes)]) from concatenated `mykrobe variants make-probes`
    output (FASTA text, bytes or a path).  A record whose name starts with "ref-" belongs to variant NAME, the text between "ref-"
    and the first "?" or whitespace; it opens a new variant unless the open one has that name.  Every following record that does not
    start with "ref-" is an alt probe of the open variant.  The probes come back grouped: variant by variant, its ref probes, then
    its alt probes; allele_of is 2 v for a ref probe of variant v and 2 v + 1 for an alt probe."""
    if isinstance(fasta, bytes):
        fasta = fasta.decode()
    if isinstance(fasta, str) and not fasta.lstrip().startswith(">") and os.path.exists(fasta):
        recs = read_fasta(fasta)
    else:
        recs = read_fasta(io.StringIO(fasta))
    names, refs, alts = [], [], []
    for name, seq in recs:
        if name.startswith("ref-"):
            var = re.split(r"[?\s]", name[4:], maxsplit=1)[0]
            if not names or names[-1] != var:
                if var in names:
                    raise ValueError("variant %r occurs twice in the panel, with other variants in between" % var)
                names.append(var)
                refs.append([])
                alts.append([])
            refs[-1].append(seq)
        else:
            if not names:
                raise ValueError("the panel starts with %r, which is no ref- record: an alt probe needs an open variant" % name)
            alts[-1].append(seq)
    probes, allele_of = [], []
    for v in range(len(names)):
        probes += refs[v] + alts[v]
        allele_of += [2 * v] * len(refs[v]) + [2 * v + 1] * len(alts[v])
    return names, probes, np.asarray(allele_of, dtype=np.uint32)


def slices(allele_of, n_variants, row_bytes, plane_bytes):
    """[(v0, v1, probe indices, their allele_of relative to v0)]: the panel cut by variant so that both planes of a slice's variants
    (2 x row_bytes rounded up to whole 8-byte words each) fit plane_bytes -- at least one variant per slice.  A probe goes to its
    variant's slice only; NONE probes go nowhere."""
    allele_of = np.asarray(allele_of, dtype=np.uint32)
    per_variant = 2 * ((int(row_bytes) + 7) // 8) * 8
    step = max(int(plane_bytes) // per_variant, 1)
    out = []
    variant = np.where(allele_of == NONE, np.int64(-1), allele_of.astype(np.int64) >> 1)
    for v0 in range(0, int(n_variants), step):
        v1 = min(v0 + step, int(n_variants))
        idx = np.flatnonzero((variant >= v0) & (variant < v1))
        out.append((v0, v1, idx, (allele_of[idx] - np.uint32(2 * v0)).astype(np.uint32)))
    return out


def calls(ref_planes, alt_planes, n_cols, excluded=()):
    """uint8[n_variants, n_cols] of indexes into GENOTYPES from the two planes (uint8[n_variants, ceil(n_cols / 8)], row format): 0/0
    ref only, 0/1 both, 1/1 alt only, ./. neither.  An excluded column is ./. whatever the planes hold."""
    r = np.unpackbits(np.asarray(ref_planes, dtype=np.uint8), axis=1)[:, :n_cols].astype(bool)
    a = np.unpackbits(np.asarray(alt_planes, dtype=np.uint8), axis=1)[:, :n_cols].astype(bool)
    out = np.full(r.shape, 3, np.uint8)
    out[r & ~a] = 0
    out[r & a] = 1
    out[a & ~r] = 2
    ex = np.asarray(excluded, dtype=np.int64).reshape(-1)
    out[:, ex[(ex >= 0) & (ex < n_cols)]] = 3
    return out


def result(names, variant_counts, sample_counts, allele_probes, name_of, excluded=(), call_matrix=None):
    """What BIGSI.genotype_panel returns.  variant_counts uint32[n, 4], sample_counts uint32[n_cols, 2], allele_probes uint32[n, 2];
    call_matrix: calls(), or None for a summary (the variants then carry no "calls").  name_of: colour -> name, None for a colour the
    metadata has no record of (it is then left out of "calls" and reported by its colour alone in "samples")."""
    variant_counts, sample_counts, allele_probes = np.asarray(variant_counts), np.asarray(sample_counts), np.asarray(allele_probes)
    n_cols = sample_counts.shape[0]
    ex = set(int(c) for c in np.asarray(excluded).reshape(-1))
    col_names = [None if c in ex else name_of(c) for c in range(n_cols)]
    variants = []
    for v, name in enumerate(names):
        rec = {"name": name, "ref_probes": int(allele_probes[v, 0]), "alt_probes": int(allele_probes[v, 1]),
               "counts": {g: int(variant_counts[v, i]) for i, g in enumerate(GENOTYPES)}}
        if call_matrix is not None:
            row = call_matrix[v]
            rec["calls"] = {col_names[c]: GENOTYPES[int(row[c])] for c in np.flatnonzero(row != 3) if col_names[c] is not None}
        if rec["ref_probes"] == 0 or rec["alt_probes"] == 0:
            rec["uncallable"] = True
        variants.append(rec)
    samples = [{"sample_name": name_of(c), "colour": c, "carried": int(sample_counts[c, 0]), "called": int(sample_counts[c, 1])}
               for c in range(n_cols) if c not in ex]
    return {"variants": variants, "samples": samples}


def to_json(res):
    return json.dumps(res)


def _cell(s):
    return re.sub(r"[\t\r\n]", " ", str(s))


def to_tsv(res, summary_only=False):
    """The matrix: header variant<TAB>sample..., one line per variant, cells 0/0 0/1 1/1 ./. (the samples of res["samples"], in colour
    order).  summary_only: per variant its counts and probes, then per sample carried / called."""
    if summary_only:
        lines = ["variant\tref_probes\talt_probes\t" + "\t".join(GENOTYPES)]
        lines += ["%s\t%d\t%d\t%s" % (_cell(v["name"]), v["ref_probes"], v["alt_probes"], "\t".join(str(v["counts"][g]) for g in GENOTYPES)) for v in res["variants"]]
        lines.append("sample\tcolour\tcarried\tcalled")
        lines += ["%s\t%d\t%d\t%d" % (_cell(s["sample_name"]), s["colour"], s["carried"], s["called"]) for s in res["samples"]]
        return "\n".join(lines)
    names = [s["sample_name"] for s in res["samples"]]
    lines = ["variant\t" + "\t".join(_cell(n) for n in names)]
    for v in res["variants"]:
        lines.append(_cell(v["name"]) + "\t" + "\t".join(v["calls"].get(n, "./.") for n in names))
    return "\n".join(lines)
