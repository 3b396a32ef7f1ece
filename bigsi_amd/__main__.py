"""`python -m bigsi_amd <command>`: the query-side commands of the reference CLI (bigsi/__main__.py:103-320) on the
hip-hbm backend.  argparse instead of hug; same command names, arguments and output text."""
import argparse
import json
import os
import sys

import yaml

from . import BIGSI
from .bitrow import BitRow
from .frontend import bulk_search, read_fasta, search, variant_search
from .graph.bigsi import DEFAULT_CONFIG
from .storage import get_storage
from .utils import seq_to_kmers


def positive_int(text):
    """argparse type of --limit: an integer >= 1."""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("invalid int value: %r" % text)
    if n < 1:
        raise argparse.ArgumentTypeError("must be >= 1, got %d" % n)
    return n


def non_negative_int(text):
    """argparse type of --margin: an integer >= 0."""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("invalid int value: %r" % text)
    if n < 0:
        raise argparse.ArgumentTypeError("must be >= 0, got %d" % n)
    return n


def get_config_from_file(config_file):            # __main__.py:86-94
    config_file = config_file or os.environ.get("BIGSI_CONFIG")
    if not config_file:
        return DEFAULT_CONFIG
    with open(config_file) as f:
        return yaml.safe_load(f)


def build_parser():
    """(the argument parser, and the sub-parsers of `search` and `bulk_search` for their own error messages)"""
    p = argparse.ArgumentParser(prog="bigsi_amd")
    sub = p.add_subparsers(dest="cmd", required=True)

    def common(sp):
        sp.add_argument("--config", "-c", default=None)
        return sp

    def shardable(sp):
        sp.add_argument("--sharded", action="store_true",
                        help="the index is spread by column range over the ranks of a `python -m torch.distributed.run` launch "
                             "(one process per GPU); rank 0 prints")
        sp.add_argument("--out", "-o", default=None,
                        help="with --sharded: write the text to this file instead of stdout (transport libraries announce "
                             "themselves on stdout)")
        return sp

    def limited(sp, text="only the first N results of every record (the best N samples: most k-mers found, ties to the lowest colour)"):
        sp.add_argument("--limit", type=positive_int, default=None, metavar="N", help=text)
        return sp

    sp = limited(shardable(common(sub.add_parser("search"))))
    sp.add_argument("seq")
    sp.add_argument("--threshold", "-t", type=float, default=1.0)
    sp.add_argument("--score", action="store_true")
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    search_parser = sp
    sp = limited(shardable(common(sub.add_parser("bulk_search"))))
    sp.add_argument("fasta")
    sp.add_argument("--threshold", "-t", type=float, default=1.0)
    sp.add_argument("--score", action="store_true")
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    bulk_parser = sp
    sp.add_argument("--stream", action="store_true")
    sp = common(sub.add_parser("variant_search"))
    sp.add_argument("reference")
    sp.add_argument("ref")
    sp.add_argument("pos", type=int)
    sp.add_argument("alt")
    sp.add_argument("--gene", "-g", default=None)
    sp.add_argument("--genbank", "-b", default=None)
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    sp.add_argument("--probes", default=None, help="output of `mykrobe variants make-probes` for this variant (skips calling it)")
    sp = common(sub.add_parser("bloom", help="Bloom filter of the k-mers of a Cortex .ctx graph, a FASTA file or a one-k-mer-per-line text file"))
    sp.add_argument("infile")
    sp.add_argument("outfile")
    sp.add_argument("--min-count", type=int, default=None, metavar="C",
                    help="FASTQ / FASTA reads: keep the k-mers seen at least C times, counted exactly on the device (k <= 32; default 1 for FASTQ)")
    sp.add_argument("--spectrum", default=None, metavar="FILE", help="FASTQ / FASTA reads: also write the k-mer abundance spectrum, 256 lines of count<TAB>distinct")
    sp = shardable(common(sub.add_parser("build")))
    sp.add_argument("--bloomfilters", "-b", action="append", default=[])
    sp.add_argument("--samples", "-s", action="append", default=[])
    sp.add_argument("--from_file", default=None, help="TSV of bloomfilter path <tab> sample name (bigsi/__main__.py:139-156)")
    sp = common(sub.add_parser("merge", help="append the samples of the index described by MERGE_CONFIG (bigsi/__main__.py:173-181)"))
    sp.add_argument("merge_config")
    sp = common(sub.add_parser("insert"))
    sp.add_argument("bloomfilter")
    sp.add_argument("sample")
    common(sub.add_parser("delete"))
    sp = common(sub.add_parser("hold", help="load the index and keep it resident in HBM for OTHER processes: writes an attach file (hipIpc handle + "
                                            "metadata); `search` / `bulk_search` with storage-config {attach: FILE} then open it in milliseconds"))
    sp.add_argument("--handle", default=None, help="the attach file (default: storage-config `export`, else <filename>.attach)")
    sp.add_argument("--seconds", type=float, default=None, help="exit after this long (default: until SIGTERM / SIGINT)")
    sp.add_argument("--until-eof", action="store_true", help="also exit when stdin ends (a parent process that holds the other end of a pipe)")
    sp = common(sub.add_parser("import-bdb", help="load an existing BerkeleyDB index (v0.3 file, or a v0.1 directory with graph + metadata) into HBM"))
    sp.add_argument("path")
    sp = common(sub.add_parser("stats", help="how full every sample's Bloom filter is: bits set, fill, the k-mer false-positive rate it implies, estimated distinct k-mers"))
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    sp = limited(common(sub.add_parser("similar", help="the samples whose Bloom filters share most with SAMPLE's: bits shared, Jaccard index, containment")),
                 "only the N most similar samples (highest Jaccard index, ties to the lowest colour)")
    sp.add_argument("sample")
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    sp = common(sub.add_parser("vacuum", help="remove the columns of deleted samples from the matrix and renumber the samples that stay"))
    sp.add_argument("--no-shrink", action="store_true", help="keep the row stride (and the HBM) the index had before")
    sp = common(sub.add_parser("extract", help="a new index, described by TO_CONFIG, of the named samples of this one, in this one's colour order"))
    sp.add_argument("to_config")
    sp.add_argument("--samples", "-s", action="append", default=[], metavar="NAME")
    sp.add_argument("--samples-file", default=None, metavar="FILE", help="one sample name per line")
    sp = common(sub.add_parser("fold", help="the same index under a Bloom filter of m / FACTOR bits (rows ORed together on the device, no source data needed): "
                                            "into the index TO_CONFIG describes, or --in-place"))
    sp.add_argument("to_config", nargs="?", default=None, help="config of the folded index (with --in-place: the config to use from now on)")
    sp.add_argument("--factor", type=int, required=True, metavar="D", help="a divisor of m (--dry-run lists the ones that exist)")
    sp.add_argument("--in-place", action="store_true", help="fold this index itself; TO_CONFIG must name the same storage with m = m / D")
    sp.add_argument("--dry-run", action="store_true", help="touch nothing: print the valid factors near D and the ESTIMATED fill / false-positive rate per sample")
    sp.add_argument("--no-trim", action="store_true", help="with --in-place: keep the allocation (and the HBM) the index had before")
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    sp = common(sub.add_parser("prevalence", help="for every k-mer position of SEQ (or of every record of a FASTA file): how many samples hold the k-mer, "
                                                  "and how many of the named samples"))
    sp.add_argument("seq", nargs="?", default=None)
    sp.add_argument("--fasta", default=None, metavar="FILE", help="the queries: every record of a FASTA file")
    sp.add_argument("--samples", "-s", action="append", default=[], metavar="NAME", help="also count among these samples only")
    sp.add_argument("--samples-file", default=None, metavar="FILE", help="one sample name per line")
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    sp = common(sub.add_parser("collapse", help="a new index, described by TO_CONFIG, in which every group of samples of this one is one column: "
                                                "the OR of its members (the small index that is searched first)"))
    sp.add_argument("to_config")
    sp.add_argument("--groups", required=True, metavar="FILE", help="sample<TAB>group lines; a group's colour follows its first appearance")
    sp.add_argument("--keep-others", action="store_true", help="samples the file does not name stay, each as a group of its own, after the named groups")
    sp = common(sub.add_parser("consensus", help="a new index, described by TO_CONFIG, in which every group of samples of this one is one column that keeps "
                                                 "a bit only where at least P %% of the members have it (the core of the group; collapse keeps the union)"))
    sp.add_argument("to_config")
    sp.add_argument("--groups", required=True, metavar="FILE", help="sample<TAB>group lines, as for collapse")
    sp.add_argument("--percent", type=int, default=100, metavar="P", help="in [1, 100]: a group of n members needs ceil(P n / 100) of them (default 100: all)")
    sp.add_argument("--keep-others", action="store_true", help="samples the file does not name stay, each as a group of its own, after the named groups")
    sp = common(sub.add_parser("distances", help="how much every sample shares with every other: bits shared, Jaccard index and containment of every pair, "
                                                 "in one pass on the device"))
    sp.add_argument("--samples", "-s", action="append", default=[], metavar="NAME", help="only these samples (default: every sample)")
    sp.add_argument("--samples-file", default=None, metavar="FILE", help="one sample name per line")
    sp.add_argument("--against-file", default=None, metavar="FILE", help="compare with these samples instead of with the same list (one name per line)")
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    sp = common(sub.add_parser("cluster", help="groups of near-duplicate samples (single linkage over the pairs with a Jaccard index of at least T): "
                                               "what `collapse --groups` takes"))
    sp.add_argument("--min-jaccard", type=float, required=True, metavar="T", help="in (0, 1]")
    sp.add_argument("--samples", "-s", action="append", default=[], metavar="NAME", help="only these samples (default: every sample)")
    sp.add_argument("--samples-file", default=None, metavar="FILE", help="one sample name per line")
    sp.add_argument("--out", default=None, metavar="FILE", help="also write the groups as sample<TAB>group lines, the file `collapse --groups` reads")
    sp = limited(common(sub.add_parser("tally", help="over all records of a FASTA file: which samples they hit, how many records each, and how many k-mers "
                                                     "(summed on the device; no per-record results)")),
                 "only the N samples that most records hit (ties to the lowest colour)")
    sp.add_argument("fasta")
    sp.add_argument("--threshold", "-t", type=float, default=1.0)
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    sp = common(sub.add_parser("window_search", help="the samples that hold some stretch of W consecutive k-mer positions of SEQ (or of every record "
                                                     "of a FASTA file), the best window per sample and where on the query the match lies"))
    sp.add_argument("seq", nargs="?", default=None)
    sp.add_argument("--fasta", default=None, metavar="FILE", help="the queries: every record of a FASTA file")
    sp.add_argument("--window", "-w", type=int, required=True, metavar="W", help="window length in k-mer positions (1 .. 65535)")
    sp.add_argument("--threshold", "-t", type=float, default=1.0)
    sp.add_argument("--format", choices=["json", "csv"], default="json")
    sp = common(sub.add_parser("classify", help="for every record of a FASTA file: which group of samples it belongs to (the hits of each group weighed "
                                                "on the device; one line per record)"))
    sp.add_argument("fasta")
    sp.add_argument("--groups", required=True, metavar="FILE", help="sample<TAB>group lines, as for collapse; a group's id follows its first appearance")
    sp.add_argument("--threshold", "-t", type=float, default=1.0)
    sp.add_argument("--margin", type=non_negative_int, default=1, metavar="D",
                    help="assign a record hit by several groups only when the best group found at least D k-mers more than the next (default 1)")
    sp.add_argument("--others", default=None, metavar="NAME", help="samples the file does not name form one more group called NAME")
    sp.add_argument("--format", choices=["tsv", "json"], default="tsv")
    sp.add_argument("--summary-only", action="store_true", help="reads per group, ambiguous, unclassified and skipped only")
    sp = common(sub.add_parser("associate", help="for every record of a FASTA file (unitigs, genes, probes): how many samples of each group hold it, "
                                                 "with prevalence, odds ratio and chi-square per group (counted on the device; one line per record)"))
    sp.add_argument("fasta")
    sp.add_argument("--groups", required=True, metavar="FILE", help="sample<TAB>group lines, as for collapse; a group's id follows its first appearance")
    sp.add_argument("--threshold", "-t", type=float, default=1.0)
    sp.add_argument("--others", default=None, metavar="NAME", help="samples the file does not name form one more group called NAME")
    sp.add_argument("--min-af", type=float, default=None, metavar="F",
                    help="drop the records held by less than F or more than 1 - F of the grouped samples (0 .. 0.5)")
    sp.add_argument("--format", choices=["tsv", "json"], default="tsv")
    sp = common(sub.add_parser("genotype", help="every sample's call (0/0, 0/1, 1/1, ./.) for a panel of variants: concatenated `mykrobe variants make-probes` "
                                                "output, ref- records opening a variant (the probes are ORed into one bit plane per allele on the device)"))
    sp.add_argument("panel")
    sp.add_argument("--threshold", "-t", type=float, default=1.0)
    sp.add_argument("--format", choices=["tsv", "json"], default="tsv")
    sp.add_argument("--summary-only", action="store_true", help="per-variant counts and per-sample carried / called only (the planes are never downloaded)")
    sp = common(sub.add_parser("typing", help="which allele of each locus every sample carries (MLST, cgMLST, serotype or resistance-gene typing): a FASTA scheme of "
                                              "allele records named locus_allele; per (locus, sample) the record with the highest fraction of its k-mers found is taken on the device"))
    sp.add_argument("scheme")
    sp.add_argument("--loci-map", default=None, metavar="FILE", help="record<TAB>locus lines: the locus of the records named there (default: the record name up to its last _)")
    sp.add_argument("--profiles", default=None, metavar="FILE", help="a PubMLST profiles table (ST<TAB>locus...): adds the sequence type of every sample")
    sp.add_argument("--threshold", "-t", type=float, default=1.0)
    sp.add_argument("--format", choices=["tsv", "json"], default="tsv")
    sp.add_argument("--summary-only", action="store_true", help="per-locus and per-sample counts only (the cells are never downloaded)")
    for name in ("vacuum", "extract", "fold", "prevalence", "collapse", "consensus", "distances", "cluster", "tally", "window_search", "classify", "associate", "genotype", "typing"):          # (named so that the refusal says why)
        sub.choices[name].add_argument("--sharded", action="store_true", help=argparse.SUPPRESS)
    return p, search_parser, bulk_parser


def stats_text(index, fmt="json"):
    """`stats`: BIGSI.sample_stats() as JSON, or CSV with a header line."""
    from .stats import STATS_KEYS, to_csv
    rows = index.sample_stats()
    return to_csv(rows, STATS_KEYS) if fmt == "csv" else json.dumps(rows)


def similar_text(index, sample, limit=None, fmt="json"):
    """`similar`: BIGSI.similar_samples(sample, limit) as JSON, or CSV with a header line."""
    from .stats import SIMILAR_KEYS, to_csv
    rows = index.similar_samples(sample, limit=limit)
    return to_csv(rows, SIMILAR_KEYS) if fmt == "csv" else json.dumps(rows)


def distances_text(index, samples=None, against=None, fmt="json"):
    """`distances`: BIGSI.sample_distances as JSON (the matrices as lists of rows), or as CSV: the three matrices one after the
    other, each under a line with its name, rows and columns under the sample names."""
    from .distances import to_matrix_csv
    d = index.sample_distances(samples, against)
    keys = ("bits_shared", "jaccard", "containment")
    if fmt == "csv":
        return "\n".join("# %s\n%s" % (k, to_matrix_csv(d[k], d["samples"], d["against"])) for k in keys)
    return json.dumps({"samples": d["samples"], "against": d["against"], **{k: d[k].tolist() for k in keys}})


def cluster_text(index, min_jaccard, samples=None, out=None):
    """`cluster`: BIGSI.cluster_samples as JSON (group -> members); --out FILE also gets it as the lines `collapse --groups` reads."""
    from .distances import groups_to_tsv
    groups = index.cluster_samples(min_jaccard, samples)
    if out:
        with open(out, "w") as f:
            f.write(groups_to_tsv(groups))
    return json.dumps(groups)


def vacuum_text(index, shrink=True):
    """`vacuum`: BIGSI.vacuum, then the snapshot (the only thing the next process sees)."""
    before = index.num_samples
    removed = index.vacuum(shrink=shrink)
    if removed:
        index.storage.sync()
    return json.dumps({"result": "removed %d of %d samples" % (removed, before), "removed": removed, "num_samples": index.num_samples})


def extract_names(a):
    """The sample names of an `extract` command line: -s NAME ... XOR --samples-file FILE (one name per line)."""
    if a.samples_file and a.samples:
        raise ValueError("You can only name samples via --samples-file or -s, but not both")
    if a.samples_file:
        with open(a.samples_file) as f:
            return [line.strip() for line in f if line.strip()]
    return list(a.samples)


def extract_text(index, config_name, to_config_name, names):
    """`extract`: BIGSI.extract into the index TO_CONFIG describes (it syncs its own snapshot)."""
    new = index.extract(get_config_from_file(to_config_name), names)
    return json.dumps({"result": "extracted %d of %d samples from %s into %s." % (new.num_samples, index.num_samples, config_name, to_config_name),
                       "num_samples": new.num_samples})


def collapse_groups(path):
    """The (sample, group) pairs of a `collapse --groups FILE`: one sample<TAB>group per line, blank lines skipped."""
    pairs = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            cells = line.split("\t")
            if len(cells) != 2 or not cells[0].strip() or not cells[1].strip():
                raise ValueError("%s line %d: expected sample<TAB>group, got %r" % (path, no, line))
            pairs.append((cells[0].strip(), cells[1].strip()))
    return pairs


def collapse_text(index, config_name, to_config_name, pairs, keep_others=False):
    """`collapse`: BIGSI.collapse into the index TO_CONFIG describes (it syncs its own snapshot); the report names the membership."""
    from .collapse import DROPPED, collapse_plan
    new = index.collapse(get_config_from_file(to_config_name), pairs, keep_others=keep_others)
    names = [index.colour_to_sample(c) for c in range(index.num_samples)]
    group_of, group_names, members = collapse_plan(names, pairs, keep_others)
    from .graph.metadata import DELETION_SPECIAL_SAMPLE_NAME
    live = sum(1 for n in names if n != DELETION_SPECIAL_SAMPLE_NAME)          # (deleted samples are not counted as dropped: they were gone)
    moved = int((group_of != DROPPED).sum())
    return json.dumps({"result": "collapsed %d of %d samples from %s into %d groups in %s." % (moved, live, config_name, len(group_names), to_config_name),
                       "groups": len(group_names), "samples_in": live, "samples_dropped": live - moved, "num_samples": new.num_samples,
                       "members": dict(zip(group_names, members))})


def consensus_text(index, config_name, to_config_name, pairs, percent=100, keep_others=False):
    """`consensus`: BIGSI.consensus into the index TO_CONFIG describes (it syncs its own snapshot); collapse's report, plus the
    percentage and the number of members every group's column asks for."""
    from .collapse import DROPPED, collapse_plan
    from .consensus import group_sizes, need_of
    new = index.consensus(get_config_from_file(to_config_name), pairs, percent=percent, keep_others=keep_others)
    names = [index.colour_to_sample(c) for c in range(index.num_samples)]
    group_of, group_names, members = collapse_plan(names, pairs, keep_others)
    need = need_of(group_sizes(group_of, len(group_names)), percent)
    from .graph.metadata import DELETION_SPECIAL_SAMPLE_NAME
    live = sum(1 for n in names if n != DELETION_SPECIAL_SAMPLE_NAME)          # (deleted samples are not counted as dropped: they were gone)
    moved = int((group_of != DROPPED).sum())
    return json.dumps({"result": "consensus of %d of %d samples from %s at %d %% into %d groups in %s." % (moved, live, config_name, percent, len(group_names),
                                                                                                         to_config_name),
                       "groups": len(group_names), "samples_in": live, "samples_dropped": live - moved, "num_samples": new.num_samples,
                       "members": dict(zip(group_names, members)), "percent": percent, "min_members": dict(zip(group_names, (int(x) for x in need)))})


# k-mer positions of one device call of `prevalence --fasta` (a few bounded batches instead of one of any size: the device keeps a
# partial count and a result per position)
PREVALENCE_BATCH_POSITIONS = 1 << 20


def prevalence_text(index, queries, samples=None, fmt="json"):
    """`prevalence`: BIGSI.kmer_prevalence_many over the queries, in device calls of at most PREVALENCE_BATCH_POSITIONS k-mer
    positions (a single longer query is a call of its own).  JSON: the dicts, each with its "query" first; CSV:
    record,pos,kmer,samples,in_subset with one line per k-mer position."""
    from .prevalence import to_csv
    k = int(index.kmer_size)
    records, chunk, load = [], [], 0
    for q in list(queries) + [None]:
        n = 0 if q is None else max(len(q) - k + 1, 0)
        if chunk and (q is None or load + n > PREVALENCE_BATCH_POSITIONS):
            records.extend(index.kmer_prevalence_many(chunk, samples=samples))
            chunk, load = [], 0
        if q is not None:
            chunk.append(q)
            load += n
    if fmt == "csv":
        return to_csv(records, queries, k)
    return json.dumps([dict({"query": q}, **r) for q, r in zip(queries, records)])


def tally_text(index, queries, threshold=1.0, limit=None, fmt="json"):
    """`tally`: BIGSI.tally over the queries; JSON: the record; CSV: sample_name,colour,queries_hit,kmers_found, one line per sample."""
    from .tally import to_csv, to_json
    rec = index.tally(queries, threshold=threshold, limit=limit)
    return to_csv(rec) if fmt == "csv" else to_json(rec)


def classify_text(index, records, pairs, threshold=1.0, margin=1, others=None, fmt="tsv", summary_only=False):
    """`classify`: BIGSI.classify over the (name, sequence) records of a FASTA file.  TSV: name, verdict, group, best_found, num_kmers,
    second group, second_found, best sample -- one line per record, the summary behind them as `# key<TAB>value` lines; JSON: the
    result, each record with its "name" first."""
    from .classify import to_json, to_tsv
    names = [n for n, _ in records]
    res = index.classify([s for _, s in records], pairs, threshold=threshold, margin=margin, others=others)
    return to_json(res, names, summary_only) if fmt == "json" else to_tsv(res, names, summary_only)


def associate_text(index, records, pairs, threshold=1.0, others=None, min_af=None, fmt="tsv"):
    """`associate`: BIGSI.associate over the (name, sequence) records of a FASTA file.  TSV: name, num_kmers, samples_hit, then per
    group <group>:hit, :prevalence, :log2_odds, :chi2, :p -- one line per kept record, `# dropped<TAB>n` behind them; JSON: the result,
    each record with its "name" first."""
    from .associate import to_json, to_tsv
    names = [n for n, _ in records]
    res = index.associate([s for _, s in records], pairs, threshold=threshold, others=others, min_af=min_af)
    return to_json(res, names) if fmt == "json" else to_tsv(res, names)


def genotype_text(index, panel, threshold=1.0, fmt="tsv", summary_only=False):
    """`genotype`: BIGSI.genotype_panel over a panel file.  TSV: the matrix -- header variant<TAB>sample..., cells 0/0 0/1 1/1 ./. --, or
    with --summary-only the per-variant counts and the per-sample carried / called; JSON: the result."""
    from .genotype import to_json, to_tsv
    res = index.genotype_panel(panel, threshold=threshold, summary_only=summary_only)
    return to_json(res) if fmt == "json" else to_tsv(res, summary_only)


def typing_text(index, scheme, threshold=1.0, fmt="tsv", summary_only=False, profiles=None, loci_map=None):
    """`typing`: BIGSI.type_samples over a scheme file.  TSV: the matrix -- header sample<TAB>[ST<TAB>]locus..., a cell the allele of an
    exact call, allele~fraction of a partial one, - without a call --, or with --summary-only the per-locus and per-sample counts;
    JSON: the result."""
    from .locus_typing import to_json, to_tsv
    res = index.type_samples(scheme, threshold=threshold, profiles=profiles, summary_only=summary_only, loci_map=loci_map)
    return to_json(res) if fmt == "json" else to_tsv(res, summary_only)


def window_search_text(index, queries, window, threshold=1.0, fmt="json"):
    """`window_search`: BIGSI.search_windows_many over the queries, one device call per query (a long query is a call's worth of work,
    and the device keeps counters per sequence).  JSON: the dicts, each with its "query" first; CSV: record,<result fields>, one line
    per reported sample."""
    from .window import to_csv, to_json
    queries = list(queries)
    recs = [index.search_windows(q, window, threshold) for q in queries]
    return to_csv(recs) if fmt == "csv" else to_json(recs, queries)


def fold_dry_run_text(index, factor, fmt="json"):
    """`fold --dry-run`: nothing is touched.  The valid factors whose folded size is nearest to the one asked for, and per sample the
    fill and k-mer false-positive rate the balls-in-bins model PREDICTS (fold.fold_estimate) -- estimates, labelled as such; the exact
    figures are `stats` of the folded index."""
    from .fold import FOLD_KEYS, divisors_near, fold_estimate_rows
    from .stats import to_csv
    m, h = int(index.bloomfilter_size), int(index.num_hashes)
    valid = factor >= 1 and m % factor == 0
    near = divisors_near(m, max(m // max(factor, 1), 1))
    rows = fold_estimate_rows(index.sample_stats(), m, h, factor) if valid else []
    if fmt == "csv":
        return to_csv(rows, FOLD_KEYS)
    return json.dumps({"m": m, "factor": factor, "valid": valid, "new_m": m // factor if valid else None,
                       "factors_near": [list(fm) for fm in near],
                       "note": "est_fill and est_kmer_fpr are model estimates (independent bits); `stats` of the folded index gives the exact figures",
                       "estimate": rows})


def fold_check_in_place(config, new_config, factor):
    """--in-place: the config to use from now on must describe THIS storage under m / factor; checked before anything is touched."""
    from .fold import fold_plan
    new_m = fold_plan(int(config["m"]), factor)
    for key, want in (("m", new_m), ("h", config["h"]), ("k", config["k"])):
        if int(new_config[key]) != int(want):
            raise ValueError("the new config must say %s = %d, it says %d" % (key, want, new_config[key]))
    if new_config.get("storage-engine") != config.get("storage-engine"):
        raise ValueError("the new config must name the same storage-engine")
    a, b = dict(config.get("storage-config") or {}), dict(new_config.get("storage-config") or {})
    for key in ("name", "filename", "device", "devices"):
        if a.get(key) != b.get(key):
            raise ValueError("--in-place: the new config must describe the same storage (storage-config %s: %r vs %r)" % (key, a.get(key), b.get(key)))
    return new_m


def fold_text(config, config_name, to_config_name, factor, in_place=False, trim=True):
    """`fold`: BIGSI.fold_into the index TO_CONFIG describes (it syncs its own snapshot), or --in-place BIGSI.fold and the snapshot."""
    new_config = get_config_from_file(to_config_name)
    if in_place:
        fold_check_in_place(config, new_config, factor)
        index = BIGSI(config)
        old_m = int(index.bloomfilter_size)
        out = index.fold(factor, trim=trim)
        index.storage.sync()
        return json.dumps(dict(out, result="folded %s by %d in place: %d rows -> %d rows; use %s from now on." % (config_name, factor, old_m, out["m"], to_config_name)))
    index = BIGSI(config)
    new = index.fold_into(new_config, factor)
    return json.dumps({"result": "folded %s by %d into %s: %d rows -> %d rows." % (config_name, factor, to_config_name, int(index.bloomfilter_size), int(new.bloomfilter_size)),
                       "m": int(new.bloomfilter_size), "factor": factor, "num_samples": new.num_samples})


def main(argv=None):
    p, search_parser, bulk_parser = build_parser()
    a = p.parse_args(argv)
    if getattr(a, "sharded", False) and getattr(a, "limit", None) is not None:
        (search_parser if a.cmd == "search" else bulk_parser).error("--limit is not available with --sharded (use a single index or storage-config devices)")
    config = get_config_from_file(a.config)

    if getattr(a, "sharded", False) and a.cmd in ("vacuum", "extract", "collapse", "consensus"):
        p.error("%s is not available with --sharded: column shards have a fixed width (use a single index)" % a.cmd)
    if getattr(a, "sharded", False) and a.cmd == "fold":
        p.error("fold is not available with --sharded: folding column shards is not implemented (use a single index)")
    if getattr(a, "sharded", False) and a.cmd == "prevalence":
        p.error("prevalence is not available with --sharded: the per-shard sweep plus a host sum is not implemented (use a single index)")
    if getattr(a, "sharded", False) and a.cmd in ("distances", "cluster"):
        p.error("%s is not available with --sharded: pairs of samples on different shards are not implemented (use a single index)" % a.cmd)
    if getattr(a, "sharded", False) and a.cmd == "tally":
        p.error("tally is not available with --sharded: the per-shard sums plus a host merge are not implemented (use a single index)")
    if getattr(a, "sharded", False) and a.cmd == "classify":
        p.error("classify is not available with --sharded: a group's samples may lie on several shards and the per-shard records plus a host merge "
                "are not implemented (use a single index)")
    if a.cmd == "classify":
        from .collapse import check_groups
        if not a.threshold <= 1:
            p.error("classify: the threshold must be <= 1, got %r" % (a.threshold,))
        try:
            classify_pairs = collapse_groups(a.groups)
            check_groups(classify_pairs)
        except (OSError, ValueError) as e:
            p.error("classify --groups: %s" % e)
    if getattr(a, "sharded", False) and a.cmd == "associate":
        p.error("associate is not available with --sharded: a group's samples may lie on several shards and the per-shard counts plus a host merge "
                "are not implemented (use a single index)")
    if a.cmd == "associate":
        from .collapse import check_groups
        if not a.threshold <= 1:
            p.error("associate: the threshold must be <= 1, got %r" % (a.threshold,))
        if a.min_af is not None and not 0.0 <= a.min_af <= 0.5:
            p.error("associate: --min-af must be within 0 .. 0.5, got %r" % (a.min_af,))
        try:
            associate_pairs = collapse_groups(a.groups)
            check_groups(associate_pairs)
        except (OSError, ValueError) as e:
            p.error("associate --groups: %s" % e)
    if getattr(a, "sharded", False) and a.cmd == "genotype":
        p.error("genotype is not available with --sharded: the per-shard planes plus a host merge are not implemented (use a single index)")
    if a.cmd == "genotype":
        if not a.threshold <= 1:
            p.error("genotype: the threshold must be <= 1, got %r" % (a.threshold,))
        try:
            with open(a.panel) as f:
                genotype_panel = f.read()
            from .genotype import parse_panel
            if not parse_panel(genotype_panel)[0]:
                raise ValueError("no variant in it")
        except (OSError, ValueError) as e:
            p.error("genotype: the panel %s: %s" % (a.panel, e))
    if getattr(a, "sharded", False) and a.cmd == "typing":
        p.error("typing is not available with --sharded: the per-shard cells plus a host merge are not implemented (use a single index)")
    if a.cmd == "typing":
        if not a.threshold <= 1:
            p.error("typing: the threshold must be <= 1, got %r" % (a.threshold,))
        try:
            from .locus_typing import parse_loci_map, parse_profiles, parse_scheme
            with open(a.scheme) as f:
                typing_scheme = f.read()
            typing_map = typing_profiles = None
            if a.loci_map is not None:
                with open(a.loci_map) as f:
                    typing_map = parse_loci_map(f.read() + "\n")
            typing_loci = parse_scheme(typing_scheme, typing_map)[0]
            if not typing_loci:
                raise ValueError("no record in it")
            if a.profiles is not None:
                with open(a.profiles) as f:
                    typing_profiles = f.read() + "\n"
                parse_profiles(typing_profiles, typing_loci)
        except (OSError, ValueError) as e:
            p.error("typing: the scheme %s: %s" % (a.scheme, e))
    if getattr(a, "sharded", False) and a.cmd == "window_search":
        p.error("window_search is not available with --sharded: the per-shard sweep is not implemented (use a single index)")
    if a.cmd == "window_search" and (a.seq is None) == (a.fasta is None):
        p.error("window_search takes SEQ or --fasta FILE (one of them)")
    if a.cmd == "window_search":
        from .window import check_args
        try:
            check_args(a.window, a.threshold)
        except ValueError as e:
            p.error(str(e))
    if a.cmd == "prevalence" and (a.seq is None) == (a.fasta is None):
        p.error("prevalence takes SEQ or --fasta FILE (one of them)")
    if a.cmd == "fold" and not a.dry_run and not a.to_config:
        p.error("fold needs TO_CONFIG (the config of the folded index) unless --dry-run is given")
    if getattr(a, "sharded", False):
        return sharded_main(a, config)
    if a.cmd == "search":
        print(search(BIGSI(config), a.seq, a.threshold, a.score, a.format, limit=a.limit))
    elif a.cmd == "bulk_search":
        text = bulk_search(BIGSI(config), a.fasta, a.threshold, a.score, a.format, a.stream, limit=a.limit)
        if text is not None:
            print(text)
    elif a.cmd == "variant_search":
        print(variant_search(BIGSI(config), a.reference, a.ref, a.pos, a.alt, a.gene, a.genbank, a.format, a.probes))
    elif a.cmd == "bloom":
        first = bloom_input_head(a.infile, a.min_count is not None or a.spectrum is not None)
        min_count = bloom_counter_route(p, first, a.min_count, a.spectrum, config["k"])          # (refusals come before any device work)
        if min_count is not None:
            from .kmercount import bloom_from_reads, spectrum_text
            spectra = [] if a.spectrum else None
            row = bloom_from_reads(config, [os.path.abspath(a.infile)], min_count, spectrum_out=spectra)
            if a.spectrum:
                with open(a.spectrum, "w") as f:
                    f.write(spectrum_text(spectra[0]))
        else:
            if first == b"CORTEX":                  # the reference's input: a Cortex graph (bigsi/__main__.py:120-131)
                from .cortex import extract_kmers_from_ctx
                kmers = list(extract_kmers_from_ctx(a.infile, config["k"]))
            elif first[:1] == b">":
                kmers = [km for _, s in read_fasta(a.infile) for km in seq_to_kmers(s, config["k"])]
            else:
                kmers = [l.strip() for l in open(a.infile) if l.strip()]
            row = BIGSI.bloom(config, kmers)
        with open(a.outfile, "wb") as f:
            f.write(row.tobytes())
    elif a.cmd == "build":
        paths, samples = build_inputs(a)
        build_in_slabs(config, paths, samples)
        print('{"result": "success"}')
    elif a.cmd == "merge":
        other_config = get_config_from_file(a.merge_config)
        index = BIGSI(config)
        index.merge(BIGSI(other_config))
        index.storage.sync()                        # the snapshot file is the only thing the next process sees
        print(json.dumps({"result": "merged %s into %s." % (a.merge_config, a.config)}))
    elif a.cmd == "insert":
        index = BIGSI(config)
        index.insert(BitRow.frombytes(open(a.bloomfilter, "rb").read(), config["m"]), a.sample)
        index.storage.sync()                        # persist: the reference's backends write through
        print('{"result": "success"}')
    elif a.cmd == "import-bdb":
        from . import bdb
        dst = get_storage(config)
        if os.path.isdir(a.path):
            print("rows=%d cols=%d k=%d" % bdb.import_v01_index(a.path, dst))
        else:
            print("rows=%d cols=%d" % bdb.import_index(a.path, dst))
    elif a.cmd == "delete":
        get_storage(config).delete_all()
    elif a.cmd == "stats":
        print(stats_text(BIGSI(config), a.format))
    elif a.cmd == "similar":
        print(similar_text(BIGSI(config), a.sample, a.limit, a.format))
    elif a.cmd == "vacuum":
        print(vacuum_text(BIGSI(config), not a.no_shrink))
    elif a.cmd == "extract":
        print(extract_text(BIGSI(config), a.config, a.to_config, extract_names(a)))
    elif a.cmd == "collapse":
        print(collapse_text(BIGSI(config), a.config, a.to_config, collapse_groups(a.groups), a.keep_others))
    elif a.cmd == "consensus":
        print(consensus_text(BIGSI(config), a.config, a.to_config, collapse_groups(a.groups), a.percent, a.keep_others))
    elif a.cmd == "fold":
        if a.dry_run:
            print(fold_dry_run_text(BIGSI(config), a.factor, a.format))
        else:
            print(fold_text(config, a.config, a.to_config, a.factor, a.in_place, not a.no_trim))
    elif a.cmd == "prevalence":
        queries = [a.seq] if a.fasta is None else [s for _, s in read_fasta(a.fasta)]
        names = extract_names(a)
        print(prevalence_text(BIGSI(config), queries, names or None, a.format))
    elif a.cmd == "window_search":
        queries = [a.seq] if a.fasta is None else [s for _, s in read_fasta(a.fasta)]
        print(window_search_text(BIGSI(config), queries, a.window, a.threshold, a.format))
    elif a.cmd == "tally":
        print(tally_text(BIGSI(config), [s for _, s in read_fasta(a.fasta)], a.threshold, a.limit, a.format))
    elif a.cmd == "classify":
        print(classify_text(BIGSI(config), read_fasta(a.fasta), classify_pairs, a.threshold, a.margin, a.others, a.format, a.summary_only))
    elif a.cmd == "genotype":
        print(genotype_text(BIGSI(config), genotype_panel, a.threshold, a.format, a.summary_only))
    elif a.cmd == "typing":
        print(typing_text(BIGSI(config), typing_scheme, a.threshold, a.format, a.summary_only, typing_profiles, typing_map))
    elif a.cmd == "associate":
        print(associate_text(BIGSI(config), read_fasta(a.fasta), associate_pairs, a.threshold, a.others, a.min_af, a.format))
    elif a.cmd == "distances":
        against = None
        if a.against_file:
            with open(a.against_file) as f:
                against = [line.strip() for line in f if line.strip()]
        print(distances_text(BIGSI(config), extract_names(a) or None, against, a.format))
    elif a.cmd == "cluster":
        print(cluster_text(BIGSI(config), a.min_jaccard, extract_names(a) or None, a.out))
    elif a.cmd == "hold":
        hold(config, a.handle, a.seconds, a.until_eof)
    return 0


def hold(config, handle=None, seconds=None, until_eof=False):
    """The process that keeps an index resident for others (the reference's store is a file every request and pool worker opens
    again, bigsi/__main__.py:75-80, 204-205; a 125 GB matrix should be ingested once).  Prints one line when the attach file is
    in place, then waits -- for SIGTERM / SIGINT, `seconds`, or (until_eof) the end of stdin -- removes the file and exits."""
    import signal
    import threading
    import time
    index = BIGSI(config)
    sc = config.get("storage-config", {})
    path = handle or sc.get("export") or ((sc.get("filename") or "bigsi-%s" % sc.get("name", "default")) + ".attach")
    index.storage.export_attach(path)
    print(json.dumps({"result": "holding", "attach": os.path.abspath(path), "pid": os.getpid(), "num_samples": index.num_samples}), flush=True)
    stop = threading.Event()
    for sig in (signal.SIGTERM, signal.SIGINT):
        signal.signal(sig, lambda *_: stop.set())

    def watch_stdin():
        try:
            while sys.stdin.read(4096):
                pass
        except (OSError, ValueError):
            return
        stop.set()
    if until_eof:                                       # (only then: a daemon's stdin is /dev/null, which is at its end at once)
        threading.Thread(target=watch_stdin, daemon=True).start()
    t0 = time.time()
    while not stop.wait(0.2):
        if seconds is not None and time.time() - t0 >= seconds:
            break
    try:
        os.remove(path)
    except OSError:
        pass


def bloom_input_head(path, counter_wanted=False):
    """The first six bytes of a `bloom` input: what decides its route.  A gzip file is looked into only for the k-mer counter, which
    reads .gz itself: its head is that of the text inside when that is FASTQ ('@'), or FASTA ('>') with --min-count / --spectrum given.
    Every other input -- a gzip file of anything else included -- is judged by its own bytes and takes the route it took before."""
    with open(path, "rb") as f:
        head = f.read(6)
    if head[:2] == b"\x1f\x8b":
        import gzip
        try:
            with gzip.open(path, "rb") as f:
                inner = f.read(6)
        except (OSError, EOFError):
            return head
        if inner[:1] == b"@" or (inner[:1] == b">" and counter_wanted):
            return inner
    return head


def bloom_counter_route(parser, first, min_count, spectrum, k):
    """The min_count the k-mer counter runs `bloom` with, or None for the routes of before (Cortex graph, FASTA windowed on the host, k-mer
    list).  FASTQ ('@') always goes to the counter; FASTA only when --min-count or --spectrum asks for it.  What cannot be done is
    refused through parser.error, before any device work."""
    wanted = min_count is not None or spectrum is not None
    reads = first[:1] in (b"@", b">")
    if min_count is not None and min_count < 1:
        parser.error("--min-count must be at least 1 (got %d)" % min_count)
    if wanted and not reads:
        parser.error("--min-count and --spectrum count the k-mers of reads (FASTQ or FASTA): a %s holds k-mers already"
                     % ("Cortex graph" if first == b"CORTEX" else "k-mer list"))
    if first[:1] != b"@" and not wanted:
        return None
    from .kmercount import MAX_K
    if not 1 <= int(k) <= MAX_K:
        parser.error("the k-mer counter takes k <= %d (config k = %d): FASTQ input, --min-count and --spectrum need it" % (MAX_K, int(k)))
    return 1 if min_count is None else min_count


def build_inputs(a):
    """(bloom filter paths, sample names) of a `build` command line, as the reference resolves them
    (bigsi/__main__.py:139-160): --from_file XOR -b; sample names default to the filter paths."""
    import csv
    paths, samples = list(a.bloomfilters), list(a.samples)
    if a.from_file and paths:
        raise ValueError("You can only specify blooms via from_file or bloomfilters, but not both")
    if a.from_file:
        paths, samples = [], []
        with open(a.from_file, "r") as tsv:
            for row in csv.reader(tsv, delimiter="\t"):
                paths.append(row[0])
                samples.append(row[1])
    if samples:
        assert len(samples) == len(paths)
    else:
        samples = list(paths)
    return paths, samples


def parse_size(text):
    """'4GB' / '512 MiB' / 1000 -> bytes (the reference hands config['max_build_mem_bytes'] to humanfriendly.parse_size:
    decimal multiples for kB/MB/GB, binary ones for KiB/MiB/GiB)."""
    import re
    if isinstance(text, (int, float)):
        return int(text)
    m = re.fullmatch(r"\s*([0-9.]+)\s*(?:([kmgtp])(i?)b?|b|bytes?)?\s*", str(text).lower())
    if not m:
        raise ValueError("cannot parse size %r" % (text,))
    value = float(m.group(1))
    if m.group(2):
        value *= (1024 if m.group(3) else 1000) ** ("kmgtp".index(m.group(2)) + 1)
    return int(value)


def build_in_slabs(config, paths, samples):
    """BIGSI.build with bounded host memory: the filters are read and sent to the device `max_build_mem_bytes` at a time
    (config key, as in the reference's chunked build, bigsi/cmds/build.py:43-73) -- the first slab builds the index, later slabs
    append their columns in place (the device transpose writes columns [col0, col0+n) of the resident matrix), so no
    temporary indexes and no merges are needed."""
    limit = parse_size(config["max_build_mem_bytes"]) if config.get("max_build_mem_bytes") else None
    per = (int(config["m"]) + 7) // 8
    slab = len(paths) if not limit else max(1, limit // max(per, 1))
    if limit and limit < per:
        raise ValueError("Max memory must be at least the Bloomfilter size in bytes")
    load = lambda b: BitRow.frombytes(open(b, "rb").read(), config["m"])      # noqa: E731
    index = BIGSI.build(config, [load(b) for b in paths[:slab]], samples[:slab])
    for i in range(slab, len(paths), slab):
        index.insert_many([load(b) for b in paths[i:i + slab]], samples[i:i + slab])
    index.storage.sync()
    return index


def sharded_main(a, config):
    """search / bulk_search / build on a column-sharded index: every rank runs the same command (SPMD), the device work
    and the exchange are bigsi_amd.parallel's, and only rank 0 writes to stdout."""
    import io

    from .parallel import ShardedBIGSI
    rank, world, _ = ShardedBIGSI.launch()
    if a.cmd == "build":
        paths, samples = build_inputs(a)
        sb = ShardedBIGSI.build(config, paths, samples)
        text = '{"result": "success"}'
    else:
        sb = ShardedBIGSI.open(config)
        if a.cmd == "search":
            text = search(sb, a.seq, a.threshold, a.score, a.format)
        else:
            sink = io.StringIO()
            text = bulk_search(sb, a.fasta, a.threshold, a.score, a.format, a.stream, out=sink)
            if text is None:                      # --stream: the records were printed into `sink`
                text = sink.getvalue()[:-1]
    if rank == 0:
        if a.out:
            with open(a.out, "w", newline="") as f:
                f.write(text + "\n")
        else:
            print(text)
    sb.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
