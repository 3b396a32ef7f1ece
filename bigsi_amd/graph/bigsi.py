"""`BIGSI`: the reference's index object (bigsi/graph/bigsi.py:129-275) over the hip-hbm backend.

`search()` / `lookup()` keep the reference's signatures, return shapes, ordering, rounding and error behaviour, but
the work between the query string and the hit list -- k-merise, dedupe, canonicalise, MurmurHash3, row fetch, AND,
per-sample counts, threshold, compaction -- is ONE device batch (include/bigsi_hip.h: bigsi_hip_batch_run).  The host
only assembles result dicts (names, percentages, optional score)."""
import json
import logging
import numbers

import numpy as np

from ..bitrow import BitRow, row_bytes_of
from ..bloom import _device_bloom
from ..scoring import Scorer
from ..storage import get_storage
from ..utils import seq_to_kmers
from .index import KmerSignatureIndex
from .metadata import DELETION_SPECIAL_SAMPLE_NAME, SampleMetadata

try:          # the C++ assembly of result dicts (bigsi_amd/_results.cpp, built by bigsi_amd/pyext_build.sh); the loop in _emit is its definition
    from .. import _results
except ImportError:
    _results = None

logger = logging.getLogger(__name__)

DEFAULT_NPROC = 4
MIN_UNIQUE_KMERS_IN_QUERY = 0
DEFAULT_CONFIG = {"storage-engine": "hip-hbm", "storage-config": {"name": "default"}, "k": 31, "m": 25 * 10 ** 6, "h": 3}


def check_limit(limit):
    """`limit` of search / search_batch / search_stream: None (every hit) or an int >= 1 -- checked before any device work."""
    if limit is None:
        return None
    if isinstance(limit, bool) or not isinstance(limit, numbers.Integral):
        raise TypeError("limit must be an int >= 1 or None, got %r" % (limit,))
    if limit < 1:
        raise ValueError("limit must be >= 1, got %d" % limit)
    return int(limit)


def validate_build_params(bloomfilters, samples):
    if len(bloomfilters) != len(samples):
        raise ValueError("There must be the same number of bloomfilters and sample names")


# sequences of a search_batch call up to this many bytes in all go through the C ABI's one-call entry point
ONE_CALL_BYTES = 192 << 10

# host memory one slice of scored hits may take as characters (the presence strings are the bulk of a scored result)
SCORE_SLICE_CHARS = 256 << 20


def scored_rows(rec, bits, boff, lengths, db_size):
    """Host half of a scored search: K6's records + presence bits (QueryBatch.score_hits / score_hits_end) -> one tuple per hit,
    (percent_kmers_found, the 17 fields of Scorer.score in the reference's key order, presence string); `lengths` = k-mer
    positions of every hit's sequence."""
    from ..scoring import score_columns, unpack_presence
    text = unpack_presence(bits, boff)
    starts = (boff[:-1].astype(np.int64) * 8).tolist()
    strings = [text[a:a + n] for a, n in zip(starts, np.asarray(lengths).tolist())]
    return list(zip(rec["percent_kmers_found"].tolist(), zip(*score_columns(rec, db_size)), strings))


def score_hit_rows(batch, off, colours, counts, num_kmers, n_seqs, db_size, slice_chars=None):
    """graph/bigsi.py:232-239 for every hit of a batch: the device extracts each hit's presence bits and runs
    remove_short_ones / tabulate_score / calculate_score on them (K6, QueryBatch.score_hits); the host derives the closed-form
    fields for all hits at once (scoring.score_columns) and expands the bits into the "kmer-presence" strings.  Returns one
    tuple per hit, in hit-list order: (percent_kmers_found, the 17 score fields in the reference's key order, presence string).
    Hits are processed in slices of at most `slice_chars` characters, so a low threshold on a wide index cannot ask for tens of
    GB of host memory at once."""
    slice_chars = slice_chars or SCORE_SLICE_CHARS
    off64 = off.astype(np.int64)
    per_hit = np.repeat(np.asarray(num_kmers[:n_seqs], dtype=np.int64), np.diff(off64[:n_seqs + 1]))
    first, total = int(off64[0]), int(off64[n_seqs])
    ends = np.cumsum((per_hit + 63) // 64 * 64)
    rows, lo = [], 0
    while first + lo < total:
        base = int(ends[lo - 1]) if lo else 0
        hi = max(int(np.searchsorted(ends, base + slice_chars, side="right")), lo + 1)
        part = np.clip(off, first + lo, first + hi).astype(np.uint64)          # the same hit lists, restricted to hits [lo, hi)
        rec, bits, boff = batch.score_hits(part, colours, counts, num_kmers)
        rows.extend(scored_rows(rec, bits, boff, per_hit[lo:hi], db_size))
        lo = hi
    return rows


def native_result_lists(nk, nu, off64, cols, counts, exact, names, scored, db_size, block=4096):
    """Generator over the result lists of the sequences 0 .. len(nu) - 1 of a search, built by the C++ extension (bigsi_amd/_results.cpp)
    from the arrays the C ABI returns: nk / nu uint32 per sequence, off64 int64 hit offsets, cols / counts uint32 per hit (ascending
    colours per sequence), names[c] = sample name or None (deleted: dropped), scored = None or (records, bits, bit_offsets) of K6
    (QueryBatch.score_hits_end / search_many_scored).  Same dicts as BIGSI._emit's Python loop and as search(); the caller deals with
    the queries the reference raises on.  `block` sequences are assembled per call of the extension."""
    from ..scoring import SCORE_KEYS, score_transcendentals
    n, total = len(nu), int(off64[len(nu)])
    keys = ("percent_kmers_found", "num_kmers", "num_kmers_found", "sample_name")
    nu = np.ascontiguousarray(nu, dtype=np.uint32)
    off64 = np.ascontiguousarray(off64, dtype=np.int64)
    cols = np.ascontiguousarray(cols[:total], dtype=np.uint32)
    cnts = np.ascontiguousarray(counts[:total], dtype=np.uint32) if counts is not None and len(counts) >= total else np.zeros(total, np.uint32)
    if scored is not None:
        # K6's records and presence bits go to the extension as they are; only the four fields that need numpy's exp / log10 are
        # computed here, for all hits at once (scoring.score_transcendentals)
        keys = keys + SCORE_KEYS + ("kmer-presence",)
        rec, bits, boff = scored
        rec = np.ascontiguousarray(rec[:total])
        trans = tuple(np.ascontiguousarray(c, dtype=np.float64) for c in score_transcendentals(rec, db_size))
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        boff = np.ascontiguousarray(boff[:total + 1], dtype=np.uint64)
        # (blocks of ~8 k hits: a block's dicts -- ~2 KB each with the presence string -- are then made in memory the consumer has just
        # released; 240 k hits built in one go measured 1.5x slower per dict, all of it page faults)
        lo = 0
        while lo < n:
            hi = min(n, lo + block, max(lo + 1, int(np.searchsorted(off64, off64[lo] + 8192, side="right")) - 1))
            yield from _results.build_scored(nu, off64, cols, cnts, bool(exact), names, keys, rec, bits, boff, trans, lo, hi)
            lo = hi
        return
    for lo in range(0, n, block):
        yield from _results.build(nu, off64, cols, cnts, bool(exact), names, keys, None, None, None, None, lo, min(n, lo + block))


def _fast_dict_selftest():
    """Whether the extension's direct-store route for result dicts may be used in THIS interpreter.  That route (bigsi_amd/_results.cpp:
    copies of a split-table template, values written into the copy's values array) leans on CPython 3.10's private dict layout; it is
    compiled for 3.10 only, checks every dict's table before it touches it -- and is OFF unless this test, run once at import, passes:
    one small batch of scored and plain result lists is built both ways and must be equal in every respect a consumer can see (values,
    key order, types, json text), stay equal under the same mutations (add / delete / pop / update a key, copy, pickle round trip) and
    survive a collection.  Anything unexpected -- an exception included -- leaves the portable PyDict_SetItem route in place."""
    if _results is None or not hasattr(_results, "fast_dict"):
        return False
    import copy
    import gc
    import json
    import pickle
    from ..scoring import HIT_SCORE_DTYPE

    class Name(str):          # (a sample name that is not a plain str: such dicts must stay visible to the collector)
        pass
    try:
        nk = np.array([40, 70, 33], np.uint32)
        off = np.array([0, 3, 3, 8], np.int64)
        cols = np.array([0, 2, 5, 1, 2, 3, 4, 6], np.uint32)
        cnts = np.array([40, 31, 40, 33, 20, 33, 9, 14], np.uint32)
        names = ["s0", "s1", Name("s2"), "s3", None, "s5", "s6"]
        rec = np.zeros(8, HIT_SCORE_DTYPE)
        rec["num_kmers"] = np.repeat(nk, np.diff(off))
        rec["score"], rec["min_score"], rec["max_score"] = np.arange(8) * 1.25 + 3, np.arange(8) * 0.5, np.arange(8) * 2.0 + 7
        rec["percent_kmers_found"] = np.round(100.0 * cnts / rec["num_kmers"], 2)
        rec["max_mismatches"], rec["min_mismatches"], rec["mismatches"] = 5, 1, 3
        boff = np.zeros(9, np.uint64)
        boff[1:] = np.cumsum((rec["num_kmers"].astype(np.int64) + 63) // 64 * 8)
        bits = (np.arange(int(boff[-1])) * 37 % 251).astype(np.uint8)

        def build():
            return (list(native_result_lists(nk, nk, off, cols, cnts, False, names, (rec, bits, boff), 1000)),
                    list(native_result_lists(nk, nk, off, cols, cnts, True, names, None, 1000)))

        def same(a, b):
            if len(a) != len(b) or [len(x) for x in a] != [len(x) for x in b]:
                return False
            for x, y in zip(a, b):
                for d, e in zip(x, y):
                    if type(d) is not dict or type(e) is not dict or d != e or list(d) != list(e) or [type(v) for v in d.values()] != [type(v) for v in e.values()]:
                        return False
                    if json.dumps(d) != json.dumps(e) or dict(d) != e or len(d) != len(e):
                        return False
            return True
        _results.fast_dict(False)
        slow = build()
        if not _results.fast_dict(True):
            return False
        fast = build()
        if not all(same(a, b) for a, b in zip(slow, fast)):
            raise ValueError("the two routes differ")
        for lists in (slow, fast):              # the same mutations on both
            for part in lists:
                for res in part:
                    for i, d in enumerate(res):
                        d["extra"] = [i]
                        d["num_kmers"] += 1
                        del d["sample_name"]
                        d.pop("percent_kmers_found")
                        d.update(zzz=i)
                        d.setdefault("sample_name", "again")
        gc.collect()
        if not all(same(a, b) for a, b in zip(slow, fast)):
            raise ValueError("the two routes differ after mutation")
        if pickle.loads(pickle.dumps(fast)) != slow or copy.deepcopy(fast) != slow:
            raise ValueError("the two routes differ after a round trip")
        del slow, fast
        gc.collect()
        return True
    except Exception as e:  # noqa: BLE001 -- whatever went wrong, the portable route is the answer
        logger.warning("bigsi_amd: the direct-store route for result dicts stays off (%s: %s)", type(e).__name__, e)
        _results.fast_dict(False)
        return False


FAST_DICT_ACTIVE = _fast_dict_selftest()


class _StreamTuning(object):
    """The two interpreter-wide settings a running search_stream changes -- a short thread switch interval, the cyclic collector's
    automatic passes paused -- owned by ALL live streams together: the first stream in saves and sets, the last one out restores,
    under a lock, so that streams in several threads (or nested ones) cannot restore each other's values out of order."""
    lock = __import__("threading").Lock()
    users = 0
    gc_users = 0
    interval = None
    gc_was_on = False

    @classmethod
    def enter(cls, pause_gc):
        import gc
        import sys
        with cls.lock:
            if cls.users == 0:
                cls.interval = sys.getswitchinterval()
                sys.setswitchinterval(min(cls.interval, 2e-4))
            cls.users += 1
            if pause_gc:
                if cls.gc_users == 0:
                    cls.gc_was_on = gc.isenabled()
                    if cls.gc_was_on:
                        gc.disable()
                cls.gc_users += 1
            return bool(pause_gc) and cls.gc_was_on

    @classmethod
    def leave(cls, pause_gc):
        import gc
        import sys
        with cls.lock:
            cls.users -= 1
            if cls.users == 0 and cls.interval is not None:
                sys.setswitchinterval(cls.interval)
            if pause_gc:
                cls.gc_users -= 1
                if cls.gc_users == 0 and cls.gc_was_on:
                    gc.enable()


class BigsiQueryResult(object):
    """One hit; `todict()` key order is part of the contract (tests/graph/test_end_to_end.py:114-124)."""

    def __init__(self, colour, sample_name, num_kmers_found, num_kmers):
        self.colour = colour
        self.sample_name = sample_name
        self.num_kmers_found = num_kmers_found
        self.num_kmers = num_kmers
        self.percent_kmers_found = round(100 * float(num_kmers_found) / num_kmers, 2)
        self.score = None

    def todict(self):
        out = {"percent_kmers_found": self.percent_kmers_found, "num_kmers": self.num_kmers,
               "num_kmers_found": self.num_kmers_found, "sample_name": self.sample_name}
        if self.score:
            out.update(self.score)
        return out

    def tojson(self):
        return json.dumps(self.todict())

    __repr__ = tojson

    def __eq__(self, other):
        return self.todict() == other.todict()

    def add_score(self, score):
        self.score = score


class _Done(object):
    """search_stream: a chunk whose results are already there (it held non-ASCII sequences)."""

    def __init__(self, results):
        self.results = results


class BIGSI(SampleMetadata, KmerSignatureIndex):
    def __init__(self, config=None):
        self.config = DEFAULT_CONFIG if config is None else config
        self.storage = get_storage(self.config)
        SampleMetadata.__init__(self, self.storage)
        KmerSignatureIndex.__init__(self, self.storage)
        self.min_unique_kmers_in_query = MIN_UNIQUE_KMERS_IN_QUERY
        self.scorer = Scorer(self.num_samples)

    @property
    def kmer_size(self):
        return self.config["k"]

    @property
    def nproc(self):
        return self.config.get("nproc", DEFAULT_NPROC)

    # ------------------------------------------------------------------ construction
    @classmethod
    def bloom(cls, config, kmers):
        """Bloom filter (m bits) of the canonical forms of `kmers`, built on the device."""
        device = (config.get("storage-config") or {}).get("device", 0)
        raw = _device_bloom(list(kmers), config["m"], config["h"], raw=False, device=device)
        return BitRow.frombytes(raw.tobytes(), int(config["m"]))

    @classmethod
    def bloom_from_reads(cls, config, paths_or_seqs, min_count=1):
        """Bloom filter (m bits) of the canonical k-mers that occur at least `min_count` times in raw reads, counted exactly on the
        device (bigsi_amd/kmercount.py): `paths_or_seqs` holds FASTQ / FASTA files (.gz or not; a str entry that names an existing
        file, or any os.PathLike) and sequences (every other str or bytes entry; pass sequences as bytes where a str could be mistaken
        for the name of a file in the working directory).  Needs config k <= 32; windows with a byte other than
        ACGTacgt are skipped.  With min_count=1 and ACGT-only input this is BIGSI.bloom of the reads' k-mers, bit for bit."""
        from ..kmercount import bloom_from_reads
        if isinstance(paths_or_seqs, (str, bytes)):
            raise TypeError("bloom_from_reads takes a list of files and sequences, not one of them")
        return bloom_from_reads(config, paths_or_seqs, min_count)

    @classmethod
    def build(cls, config, bloomfilters, samples):
        storage = get_storage(config)
        validate_build_params(bloomfilters, samples)
        SampleMetadata(storage).add_samples(samples)
        KmerSignatureIndex.create(storage, bloomfilters, config["m"], config["h"], config.get("low_mem_build", False))
        storage.close()
        return cls(config)

    @classmethod
    def build_from_sequences(cls, config, samples):
        """Build an index straight from sequences, no Bloom files and no transpose: `samples` maps sample name ->
        list of sequences; every k-mer of every sequence is Bloom-added to that sample's column on the device
        (k_insert_kmers = BIGSI.bloom + build of the reference, graph/bigsi.py:150-172, fused).  Same rows as
        build(config, [bloom(config, kmers of s) for s in samples], names)."""
        storage = get_storage(config)
        names = list(samples.keys())
        SampleMetadata(storage).add_samples(names)
        storage.set_integer("ksi:bloomfilter_size", config["m"])
        storage.set_integer("ksi:num_hashes", config["h"])
        storage.set_integer("number_of_rows", config["m"])
        storage.set_integer("number_of_cols", len(names))
        storage.res.ensure_open()
        storage.res.written[:] = True
        for colour, name in enumerate(names):
            seqs = [samples[name]] if isinstance(samples[name], str) else list(samples[name])
            if seqs:
                storage.insert_kmers(colour, seqs, config["k"])
        storage.sync()
        storage.close()
        return cls(config)

    def insert(self, bloomfilter, sample):
        logger.warning("Build and merge is preferable to insert in most cases")
        self._metadata_changed()
        colour = self.add_sample(sample)
        self.insert_bloom(bloomfilter, colour - 1)

    def insert_many(self, bloomfilters, samples):
        """Append several samples at once: their filters become the next columns through ONE device transpose
        (bigsi_hip_insert_columns) instead of a column-at-a-time loop.  Same result as insert() called for each in turn
        (graph/bigsi.py:244-247)."""
        validate_build_params(bloomfilters, samples)
        self._metadata_changed()
        col0 = self.num_samples
        self.add_samples(samples)
        nb = (int(self.bloomfilter_size) + 7) // 8
        arr = np.zeros((len(bloomfilters), nb), dtype=np.uint8)
        for i, bf in enumerate(bloomfilters):
            data = np.frombuffer(row_bytes_of(getattr(bf, "bitarray", bf))[0], dtype=np.uint8)[:nb]
            arr[i, : data.size] = data
        self.storage.insert_columns(col0, arr)
        self.bitmatrix.set_num_cols(max(self.bitmatrix.num_cols, col0 + len(bloomfilters)))

    def delete(self):
        for batch in self.__dict__.pop("_workspaces", {}).values():
            batch.close()
        self.storage.delete_all()

    def merge(self, bigsi):
        assert self.bloomfilter_size == bigsi.bloomfilter_size
        assert self.num_hashes == bigsi.num_hashes
        assert self.kmer_size == bigsi.kmer_size
        self._metadata_changed()
        self.merge_indexes(bigsi)
        self.merge_metadata(bigsi)

    def delete_sample(self, sample_name):
        self._metadata_changed()
        SampleMetadata.delete_sample(self, sample_name)

    def _metadata_changed(self):
        self.__dict__.pop("_excluded", None)
        self.__dict__.pop("_names", None)

    def _excluded_colours(self):
        """Colours of deleted samples (named DELETION_SPECIAL_SAMPLE_NAME), which a limited search takes out before it ranks: the
        reference drops them after ordering (graph/bigsi.py:185-190), so the first N of what is left are the same N.  One pass over the
        colours, kept until the metadata changes through this object."""
        ex = self.__dict__.get("_excluded")
        if ex is None:
            cols = []
            for c in range(self.num_samples):
                try:
                    if self.colour_to_sample(c) == DELETION_SPECIAL_SAMPLE_NAME:
                        cols.append(c)
                except KeyError:
                    pass
            ex = self.__dict__["_excluded"] = np.asarray(cols, dtype=np.uint32)
        return ex

    def _set_limit(self, batch, limit):
        batch.set_limit(limit, self._excluded_colours() if limit else None)

    def _limit_fallback(self, seqs, score, limit):
        """score=True on a query of ONE k-mer raises the reference's IndexError when it has any hit at all -- deleted samples included,
        which a limited run takes out before it counts: such a batch runs unlimited and is cut on the host."""
        return bool(limit and score and any(len(s) - self.kmer_size + 1 == 1 for s in seqs))

    # ------------------------------------------------------------------ queries
    def seq_to_kmers(self, seq):
        return seq_to_kmers(seq, self.kmer_size)

    def search(self, seq, threshold=1.0, score=False, limit=None):
        if len(seq) - self.kmer_size + 1 <= self.min_unique_kmers_in_query:
            logger.warning("Query string should contain at least %i unique kmers. Your query contained %i unique kmers, "
                           "and as a result the false discovery rate may be high. In future this will become an error."
                           % (self.min_unique_kmers_in_query, max(len(seq) - self.kmer_size + 1, 0)))
        assert threshold <= 1
        return self.search_batch([seq], threshold, score, limit=limit)[0]

    def _workspace(self, slot, seqs, ws=None):
        """Batch workspace `slot` (of `ws`, else of this index object), staged with `seqs` (created once, then only reloaded).
        search() / search_batch() use the object's slot 0; every stream generator brings its own dict, so that a search()
        made while a stream is being consumed cannot reload a batch the stream still has in flight."""
        if ws is None:
            ws = self.__dict__.setdefault("_workspaces", {})
        batch = ws.get(slot)
        if batch is None or batch.b is None or batch.storage.res is not self.storage.res:
            batch = ws[slot] = self.storage.new_batch(seqs, self.kmer_size)
        else:
            batch.reload(seqs, self.kmer_size)
        return batch

    def _launch(self, batch, threshold):
        # hit lists only: counters of non-hits are never stored; config key `early_exit: true` additionally lets an exact
        # search stop reading a query's rows once no sample can match any more (identical results)
        batch.run(threshold, sparse_counts=True, early_exit=bool(self.config.get("early_exit", False)))

    def _collect(self, batch, n_seqs, threshold, score):
        return self._collect_end(self._collect_begin(batch, n_seqs, threshold, score))

    def _collect_begin(self, batch, n_seqs, threshold, score, deferred=False):
        """First half of a batch's collection: per-query counts and hit lists to the host, the reference's errors for degenerate
        queries, and -- score=True -- the scored hits: at once (K6 through the synchronous call), or `deferred`: only queued
        (bigsi_hip_batch_score_hits_begin) for _collect_end to pick up, so that a stream can launch its next batch in between."""
        num_kmers, num_unique, _ = batch.unique()
        off, colours, counts = batch.hits()
        exact = threshold == 1.0
        if num_unique[:n_seqs].all() and int(off[n_seqs]) == 0:
            return None, n_seqs                           # the common bulk case: nothing found anywhere in the batch
        nu = num_unique[:n_seqs]
        if not nu.all():
            # the reference fails on a query without k-mers: reduce() over nothing on the exact branch
            # (utils/fncts.py:24-25), an unbound accumulator on the other (graph/bigsi.py:35-44)
            if exact:
                raise TypeError("reduce() of empty sequence with no initial value")
            raise UnboundLocalError("local variable 'cumsum' referenced before assignment")
        off64 = off.astype(np.int64)
        scored = None
        if score:
            if ((np.diff(off64[:n_seqs + 1]) > 0) & (num_kmers[:n_seqs] == 1)).any():
                # the reference builds a 1-D matrix from a single row and then indexes it with two subscripts
                raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
            per_hit = np.repeat(num_kmers[:n_seqs].astype(np.int64), np.diff(off64[:n_seqs + 1]))
            fits = int(((per_hit + 63) // 64 * 64).sum()) <= SCORE_SLICE_CHARS
            if deferred and not batch.group and fits:
                batch.score_hits_begin(off, colours, None if exact else counts, num_kmers)
                scored = ("pending", per_hit)
            elif _results is not None and fits and int(off[0]) == 0:
                # K6's records and presence bits as arrays: _collect_end hands them to the C++ builder (bigsi_amd/_results.cpp:
                # build_scored) instead of a tuple and a 22-key dict per hit made in Python
                scored = ("arrays", batch.score_hits(off, colours, None if exact else counts, num_kmers), num_kmers)
            else:
                scored = self._score_hits(batch, off, colours, None if exact else counts, num_kmers, n_seqs)
        return (batch, off64, colours, counts, nu, exact, scored), n_seqs

    def _collect_end(self, begun):
        state, n_seqs = begun
        if state is None:
            return [[] for _ in range(n_seqs)]
        batch, off64, colours, counts, nu, exact, scored = state
        if isinstance(scored, tuple) and scored[0] == "pending":
            rec, bits, boff = batch.score_hits_end()
            scored = scored_rows(rec, bits, boff, scored[1], self.scorer.DB_SIZE)
        elif isinstance(scored, tuple) and scored[0] == "arrays":
            (rec, bits, boff), num_kmers = scored[1], scored[2]
            total = int(off64[n_seqs])
            names = self._names_of(colours[:total], exact)
            if names is not None:
                return list(native_result_lists(num_kmers[:n_seqs], nu[:n_seqs], off64[:n_seqs + 1], colours, counts, exact, names, (rec, bits, boff), self.scorer.DB_SIZE))
            per_hit = np.repeat(num_kmers[:n_seqs].astype(np.int64), np.diff(off64[:n_seqs + 1]))
            scored = scored_rows(rec, bits, boff, per_hit, self.scorer.DB_SIZE)          # (a colour without a name: the per-record loop raises the reference's KeyError in order)
        if _results is not None and scored is None:
            # unscored: the dicts straight from the arrays (bigsi_amd/_results.cpp), as search_stream builds them
            total = int(off64[n_seqs])
            names = self._names_of(colours[:total], exact)
            if names is not None:
                return list(native_result_lists(None, nu[:n_seqs], off64[:n_seqs + 1], colours, counts, exact, names, None, self.scorer.DB_SIZE))
        out = [[] for _ in range(n_seqs)]
        for i in np.flatnonzero(np.diff(off64[:n_seqs + 1])).tolist():      # only the sequences that have hits
            lo, hi = int(off64[i]), int(off64[i + 1])
            out[i] = self._assemble(lo, colours[lo:hi], counts[lo:hi], int(nu[i]), exact, scored)
        return out

    def _score_hits(self, batch, off, colours, counts, num_kmers, n_seqs):
        return score_hit_rows(batch, off, colours, counts, num_kmers, n_seqs, self.scorer.DB_SIZE)

    def _elements_of(self, seq):
        """A non-ASCII query as the device takes it: its unique k-mers (k CHARACTERS each, utils/fncts.py:63-65) in
        first-occurrence order, canonical (character-wise, fncts.py:38-54) and UTF-8 encoded -- the bytes the reference hashes
        (bloom/bloomfilter.py:5-6) -- plus, for every position, the index of its unique k-mer."""
        from ..utils import canonical
        k, index, uniq, pos = self.kmer_size, {}, [], []
        for i in range(len(seq) - k + 1):
            km = seq[i:i + k]
            j = index.get(km)
            if j is None:
                j = index[km] = len(uniq)
                uniq.append(canonical(km).encode("utf-8"))
            pos.append(j)
        return uniq, pos

    def _search_wide(self, seqs, threshold, score, limit=None):
        """search_batch for sequences with non-ASCII characters: k-merised here, hashed / fetched / combined on the device."""
        batch = self.storage.new_element_batch([self._elements_of(s) for s in seqs])
        try:
            self._set_limit(batch, limit)
            self._launch(batch, threshold)
            return self._collect(batch, len(seqs), threshold, score)
        finally:
            batch.close()

    def search_batch(self, seqs, threshold=1.0, score=False, limit=None):
        """search() for many sequences in one device batch; a list of result lists in input order.  `limit` = N: each list is
        search(seq, threshold, score)[:N], and the device selects, exports and scores only those N (k_rank_select)."""
        limit = check_limit(limit)
        assert threshold <= 1
        with self._device_lock():          # (a search_stream being consumed has a worker thread on this index between yields)
            return self._search_batch_locked(seqs, threshold, score, limit)

    def _search_batch_locked(self, seqs, threshold, score, limit=None):
        seqs = list(seqs)
        if not seqs:
            return []
        if self._limit_fallback(seqs, score, limit):
            return [r[:limit] for r in self._search_batch_locked(seqs, threshold, score)]
        wide = [i for i, s in enumerate(seqs) if not s.isascii()]
        if wide:
            out = [None] * len(seqs)
            rest = [i for i in range(len(seqs)) if seqs[i].isascii()]
            for i, r in zip(wide, self._search_wide([seqs[i] for i in wide], threshold, score, limit)):
                out[i] = r
            if rest:
                for i, r in zip(rest, self._search_batch_locked([seqs[i] for i in rest], threshold, score, limit)):
                    out[i] = r
            return out
        if limit is None and not score and sum(map(len, seqs)) <= ONE_CALL_BYTES:
            # unscored (the reference's `search` endpoint, bigsi/__main__.py:195-209): ONE call of the C ABI -- bigsi_hip_search_batch:
            # zero-copy input, results written into pinned memory by the last kernel -- instead of reload + run + two fetches
            # (a 1 kbp query against a 125 GB index: 35 us in the C call against ~90 through the batch object)
            from .. import _lib
            flags = _lib.RUN_EARLY_EXIT if self.config.get("early_exit", False) else 0
            nk, nu, off, colours, counts = self.storage.search_batch_arrays(seqs, self.kmer_size, threshold, flags, borrow=True)
            return self._collect_end(self._check_degenerate(None, len(seqs), threshold, nk, nu, off, colours, counts))
        batch = self._workspace(0, seqs)
        self._set_limit(batch, limit)
        self._launch(batch, threshold)
        return self._collect(batch, len(seqs), threshold, score)

    def _check_degenerate(self, batch, n_seqs, threshold, num_kmers, num_unique, off, colours, counts):
        """The unscored half of _collect_begin on arrays: the reference's errors for queries without k-mers, the no-hit shortcut."""
        exact = threshold == 1.0
        if num_unique[:n_seqs].all() and int(off[n_seqs]) == 0:
            return None, n_seqs
        nu = num_unique[:n_seqs]
        if not nu.all():
            if exact:
                raise TypeError("reduce() of empty sequence with no initial value")
            raise UnboundLocalError("local variable 'cumsum' referenced before assignment")
        return (batch, off.astype(np.int64), colours, counts, nu, exact, None), n_seqs

    def search_stream(self, seqs, threshold=1.0, score=False, batch_size=None, batch_kmers=1 << 19, pause_gc=True, limit=None):
        """Generator over (sequence, results) for an arbitrarily long iterable of sequences (bulk_search, bigsi/__main__.py:261-314,
        runs one BIGSI.search per query in a fork pool).  The sequences go through the C ABI's streaming entry points --
        bigsi_hip_search_stream, or bigsi_hip_search_stream_scored with score=True: one call per slice of about 8 x `batch_kmers`
        k-mers (or 16 x `batch_size` sequences), inside which the library keeps four device batches in flight and, scored, runs
        K5 + K6 of one beside the row-AND of the next -- on a worker thread (the call holds no GIL), while this thread turns the
        arrays of the slice before into the reference's result dicts.  Results, order and the reference's errors for degenerate
        queries (raised when the offending sequence's turn comes, after everything before it was yielded) are those of search()
        per sequence.  While a stream is being consumed the index handle is in use by the worker between yields: search() /
        search_batch() / lookup() take the same lock and simply wait; do not modify the index.  `pause_gc` (default on): full
        passes of Python's cyclic garbage collector are deferred until the stream ends (see below); pass False to leave it alone.
        Exhaust the generator or .close() it: while it is suspended the process runs with the short switch interval and (pause_gc)
        without automatic collections; several streams at once share the two settings and the last one to end restores them.
        A multi-GPU (devices=[...]) index streams through its batch objects instead (_search_stream_batches), and so does a scored
        stream with a `limit` (N: every sequence's results are search(seq, threshold, score)[:N]; unscored, the streaming call
        bigsi_hip_search_stream_ranked)."""
        limit = check_limit(limit)
        assert threshold <= 1
        if self.storage.res.is_group or (limit and score):
            yield from self._search_stream_batches(seqs, threshold, score, batch_size, batch_kmers, limit)
            return
        from concurrent.futures import ThreadPoolExecutor
        from ..storage.hip_hbm import TooManyHits
        k, st, lock = self.kmer_size, self.storage, self._device_lock()

        from .. import _lib

        def pack(chunk):
            """(blob, offsets) of an all-ASCII slice -- packed on the CALLER's thread, so that the worker goes from one C call straight
            into the next -- or None: the slice then takes search_batch's route for non-ASCII text."""
            try:
                blob, soff = _lib.pack_seqs(chunk)
            except ValueError:
                return None
            return (blob, soff) if blob.isascii() else None          # (bytes among the sequences may hold anything)

        def work(chunk, packed):
            with lock:
                try:
                    if packed is None:                           # rare: answered through search_batch's non-ASCII route
                        return "done", chunk, self._search_batch_locked(chunk, threshold, score, limit)
                    if not score:
                        excluded = self._excluded_colours() if limit else None
                        return "arrays", chunk, st.search_many_packed(packed[0], packed[1], k, threshold, limit=limit, excluded=excluded)
                    try:
                        return "arrays", chunk, st.search_many_scored(None, k, threshold, max_bits=SCORE_SLICE_CHARS // 8, packed=packed)
                    except TooManyHits:                          # (a low threshold on a wide index: the batch route scores in slices)
                        return "done", chunk, self._search_batch_locked(chunk, threshold, score)
                except Exception as e:  # noqa: BLE001 -- surfaces in stream order, from emit()
                    return "error", chunk, e

        take = batch_size * 16 if batch_size else 64
        slices = self._slices(iter(seqs), take, take if batch_size else None, batch_kmers * 8, k)
        # the worker needs the GIL a few times per slice (arguments in, arrays out) while this thread assembles dicts in pure Python
        # and never lets go of it voluntarily: at the default 5 ms switch interval those handoffs cost a scored stream a third of its
        # rate (128 -> 165+ M lookups/s on BASELINE configs[4]'s shard)
        import gc
        # The stream makes two containers per sequence (the pair, the result list); every ~35 000 of them the cyclic collector
        # starts a FULL collection, which walks every object of the process -- with torch and numpy imported ~40 ms, GIL held, the
        # worker stuck at the end of its C call: a quarter of a scored stream's time (163 -> 120 ms per 24 576 queries of 1 kbp).
        # While the stream runs, full collections wait: the collector is off, and the two young generations are collected at every
        # slice boundary (cheap: only what was made since), so that cyclic garbage of the consumer does not pile up unseen.
        # Both settings are process-wide: _StreamTuning shares them between all running streams (first in sets, last out restores).
        # They are restored when the generator ends, is closed or is finalised -- a stream that is abandoned half-consumed should be
        # .close()d (a suspended generator kept alive keeps them in force).
        gc_was_on = _StreamTuning.enter(pause_gc)
        with ThreadPoolExecutor(1) as pool:
            pending = None
            try:
                for chunk in slices:
                    nxt = pool.submit(work, chunk, pack(chunk))
                    if pending is not None:
                        yield from self._emit(pending.result(), threshold, score)
                        if gc_was_on:
                            gc.collect(1)
                    pending = nxt
                if pending is not None:
                    last, pending = pending, None
                    yield from self._emit(last.result(), threshold, score)
            finally:
                _StreamTuning.leave(pause_gc)
                if pending is not None:
                    pending.result()                             # (the consumer stopped early: let the worker leave the index alone)

    # ------------------------------------------------------------------ sample statistics
    def _sample_names(self, n):
        """names[c] for the colours below n: None for a deleted sample or a colour without a record."""
        names = []
        for c in range(n):
            try:
                name = self.colour_to_sample(c)
            except KeyError:
                name = None
            names.append(None if name == DELETION_SPECIAL_SAMPLE_NAME else name)
        return names

    def sample_stats(self):
        """How full every sample's Bloom filter is: [{sample_name, colour, bits_set, fill, kmer_fpr, est_kmers}] in ascending
        colour, deleted samples dropped (bigsi_amd/stats.py: derive_sample_stats).  One sweep of the matrix on the device; nothing
        is kept between calls."""
        from ..stats import derive_sample_stats
        with self._device_lock():
            counts = self.storage.column_popcounts()
        n = min(len(counts), self.num_samples)
        return derive_sample_stats(counts, int(self.bloomfilter_size), int(self.num_hashes), self._sample_names(n))

    def similar_samples(self, query, limit=None):
        """The samples whose filters share most with `query` -- a sample name (that sample's own column, the sample itself left
        out) or a Bloom filter of this index (m bits): [{sample_name, colour, bits_shared, jaccard, containment}] by Jaccard
        index descending, ties in ascending colour, cut to `limit` (bigsi_amd/stats.py: derive_similar).  Two sweeps on the device,
        the second reading only the rows where the query filter is set; the ranking of N numbers is the host's."""
        from ..stats import derive_similar
        limit = check_limit(limit)
        m = int(self.bloomfilter_size)
        with self._device_lock():
            leave_out = None
            if isinstance(query, str):
                colour = self.sample_to_colour(query)
                if colour is None:
                    raise KeyError(query)                                        # no such sample, or a deleted one
                leave_out = colour
                mask = np.frombuffer(self.storage.get_column(colour), dtype=np.uint8)
            else:
                mask = getattr(query, "bitarray", query)
                if not isinstance(mask, (bytes, bytearray, memoryview, np.ndarray)):
                    data, nbits = row_bytes_of(mask)
                    if nbits != m:
                        raise ValueError("the Bloom filter has %d bits, the index has %d rows" % (nbits, m))
                    mask = np.frombuffer(data, dtype=np.uint8)
            masked = self.storage.column_popcounts(mask)
            counts = self.storage.column_popcounts()
        bits = np.unpackbits(np.frombuffer(bytes(mask), dtype=np.uint8) if not isinstance(mask, np.ndarray) else mask)[:m]
        n = min(len(counts), self.num_samples)
        return derive_similar(counts, int(bits.sum()), masked, self._sample_names(n), leave_out, limit)

    # ------------------------------------------------------------------ sample-to-sample distances, near-duplicate groups
    def _selected_colours(self, samples, names):
        """(names, colours) of a selection: None = every live sample in colour order; a list = those samples in the order given
        (KeyError for a name that is unknown or deleted, ValueError for an empty list)."""
        if samples is None:
            picked = [(n, c) for c, n in enumerate(names) if n is not None]
        else:
            if isinstance(samples, (str, bytes)):
                raise TypeError("samples must be a list of sample names, got %r" % type(samples))
            colour_of = {n: c for c, n in enumerate(names) if n is not None}
            picked = []
            for s in samples:
                if s not in colour_of:
                    raise KeyError(s)
                picked.append((s, colour_of[s]))
        if not picked:
            raise ValueError("no samples to compare")
        return [n for n, _ in picked], [c for _, c in picked]

    def sample_distances(self, samples=None, against=None):
        """How much every sample of `samples` shares with every sample of `against`:
            {"samples": [names], "against": [names], "bits_shared": uint64[na, nb], "jaccard": float64[na, nb], "containment": float64[na, nb]}
        (bigsi_amd/distances.py: derive_distances; the arithmetic of similar_samples, so row i holds similar_samples(samples[i])'s
        values).  samples=None: every sample that is not deleted, in colour order; against=None: the same list as `samples`, the
        square symmetric matrix.  ONE pass over the selected columns on the device (bigsi_hip_pairwise_popcounts) instead of one
        masked sweep per sample.  KeyError for a name that is unknown or deleted, ValueError for an empty list and for more than
        distances.MAX_PAIRS pairs (before any device call); multi-GPU (devices=[...]) indexes are refused."""
        from ..distances import MAX_PAIRS, derive_distances
        self._refuse_group("sample distances")
        names = self._sample_names(self.num_samples)
        a_names, a_cols = self._selected_colours(samples, names)
        b_names, b_cols = (a_names, None) if against is None else self._selected_colours(against, names)
        nb = len(a_names) if b_cols is None else len(b_cols)
        if len(a_cols) * nb > MAX_PAIRS:
            raise ValueError("%d x %d samples are more pairs than one call takes (%d)" % (len(a_cols), nb, MAX_PAIRS))
        with self._device_lock():
            inter = self.storage.pairwise_popcounts(a_cols, b_cols)
            if b_cols is None:
                set_a = set_b = inter.diagonal().copy()
            else:
                counts = self.storage.column_popcounts()
                set_a, set_b = counts[np.asarray(a_cols)], counts[np.asarray(b_cols)]
        jaccard, containment = derive_distances(inter, set_a, set_b)
        return {"samples": a_names, "against": list(b_names), "bits_shared": inter, "jaccard": jaccard, "containment": containment}

    def cluster_samples(self, min_jaccard, samples=None):
        """Groups of near-duplicates: single linkage over the pairs of sample_distances(samples) with jaccard >= min_jaccard, as an
        ordered mapping group name -> [member names] that BIGSI.collapse takes (bigsi_amd/distances.py: cluster_single_linkage --
        groups by lowest member colour under that member's name, singletons kept).  min_jaccard must be in (0, 1]: ValueError."""
        from ..distances import cluster_single_linkage
        if isinstance(min_jaccard, bool) or not isinstance(min_jaccard, (int, float)) or not 0.0 < float(min_jaccard) <= 1.0:
            raise ValueError("min_jaccard must be in (0, 1], got %r" % (min_jaccard,))
        if samples is not None:          # (groups are ordered by colour, whatever order the names came in)
            names = self._sample_names(self.num_samples)
            picked, colours = self._selected_colours(samples, names)
            if len(set(picked)) != len(picked):
                raise ValueError("a sample is named twice")
            samples = [n for _, n in sorted(zip(colours, picked))]
        d = self.sample_distances(samples)
        return cluster_single_linkage(d["jaccard"], d["samples"], float(min_jaccard))

    # ------------------------------------------------------------------ k-mer prevalence
    def kmer_prevalence_many(self, seqs, samples=None):
        """For every k-mer position of every sequence, how many samples hold the k-mer -- the transposed question of a search --
        and, with samples=[names], how many of THOSE samples: one dict per sequence,
            {"num_kmers": n, "num_unique": u (distinct window strings, counted on the host), "num_samples": |universe|, "subset_size": |subset| or None,
             "samples_with_kmer": [n ints], "subset_with_kmer": [n ints] or None}
        The universe is every sample that is not deleted.  ONE device call for all sequences (bigsi_hip_kmer_prevalence: a k-mer is
        swept once, its rows never leave the device); masks and records are bigsi_amd/prevalence.py's.  A sequence shorter than k
        gives num_kmers 0 and empty lists.  ValueError for a name that is unknown or deleted and for sequences with non-ASCII
        characters; multi-GPU (devices=[...]) indexes are refused."""
        from ..prevalence import assemble, subset_mask, universe_mask
        if isinstance(seqs, (str, bytes)):
            raise TypeError("seqs must be a list of sequences, got %r" % type(seqs))
        seqs = list(seqs)
        self._refuse_group("k-mer prevalence")
        for s in seqs:
            if not s.isascii():
                raise ValueError("k-mer prevalence takes ASCII sequences (queries with other characters are out of scope)")
        k = int(self.kmer_size)
        with self._device_lock():
            # masks as wide as the MATRIX (it may hold columns the metadata has no record of: they are in no universe)
            n_cols = int(self.storage.get_integer("number_of_cols"))
            names = self.__dict__.get("_names")          # one pass over the colours, kept until the metadata changes through this object
            if names is None or len(names) != self.num_samples:
                names = self.__dict__["_names"] = self._sample_names(self.num_samples)
            universe, n_universe = universe_mask(n_cols, names)
            subset = n_subset = None
            if samples is not None:
                subset, n_subset = subset_mask(n_cols, names, samples)
            if not seqs:
                return []
            pos, total, in_subset = self.storage.kmer_prevalence(seqs, k, universe, subset)
        return assemble(seqs, k, pos, total, in_subset, n_universe, n_subset)

    def kmer_prevalence(self, seq, samples=None):
        """kmer_prevalence_many for one sequence: its dict."""
        return self.kmer_prevalence_many([seq], samples)[0]

    # ------------------------------------------------------------------ windowed search
    def search_windows_many(self, seqs, window, threshold=1.0):
        """The local question a search cannot ask: which samples hold at least `threshold` of SOME stretch of `window` consecutive k-mer
        positions of the query, and where on the query.  One dict per sequence,
            {"num_kmers": n, "window": We = min(window, n), "min_found": ceil(We * threshold), "results": [...]}
        and per reported sample {"sample_name", "colour", "best_found", "percent_found", "best_start", "match_start", "match_end",
        "windows_passing"}: the best window's count (by POSITION: a repeated k-mer counts at each of its positions) and its lowest start,
        the bases [match_start, match_end) of the query that the passing windows span (0-based) and how many windows pass.  Results by
        best_found descending, ties to the lowest colour; deleted samples dropped.  ONE device call for all sequences
        (bigsi_hip_window_search); records are bigsi_amd/window.py's.  A sequence shorter than k has no window and no result.
        ValueError for a window outside 1 .. 65535, a threshold outside (0, 1] and sequences with non-ASCII characters; multi-GPU
        (devices=[...]) indexes are refused."""
        from ..window import assemble, check_args
        if isinstance(seqs, (str, bytes)):
            raise TypeError("seqs must be a list of sequences, got %r" % type(seqs))
        seqs = list(seqs)
        self._refuse_group("a window search")
        window, threshold = check_args(window, threshold)
        for s in seqs:
            if not s.isascii():
                raise ValueError("a window search takes ASCII sequences (queries with other characters are out of scope)")
        if not seqs:
            return []
        k = int(self.kmer_size)
        with self._device_lock():
            used, need, off, colours, records = self.storage.window_search(seqs, k, window, threshold)
            excluded = self._excluded_colours()
        return assemble(seqs, k, window, threshold, used, need, off, colours, records, self._name_of(), excluded)

    def search_windows(self, seq, window, threshold=1.0):
        """search_windows_many for one sequence: its dict."""
        return self.search_windows_many([seq], window, threshold)[0]

    def _name_of(self):
        """name_of(c) for the colours a device call reports: the sample's name, None for a column the metadata has no record of
        (it is then reported by its colour alone)."""
        n = self.num_samples

        def name_of(c):
            try:
                return self.colour_to_sample(c) if c < n else None
            except KeyError:
                return None
        return name_of

    @staticmethod
    def _check_stream_query(seqs, threshold):
        """What tally and classify_arrays refuse before any device call: one sequence in place of an iterable, a threshold above 1."""
        if isinstance(seqs, (str, bytes)):
            raise TypeError("seqs must be an iterable of sequences, got %r" % type(seqs))
        if not threshold <= 1:
            raise ValueError("threshold must be <= 1, got %r" % (threshold,))

    # ------------------------------------------------------------------ query-set tally
    def tally(self, seqs, threshold=1.0, limit=None, batch_kmers=1 << 19):
        """The question a read set poses: of these sequences, which samples do they hit, how many sequences each, and how many
        k-mers -- answered on the device (bigsi_hip_tally_add_stream: the hits of every sequence are the ones search(seq, threshold)
        reports, summed per sample behind the row-AND kernels; no hit list is built and two numbers per sample leave the device).
            {"queries": sequences counted, "kmers": their unique k-mers, "skipped": sequences shorter than k,
             "queries_with_hits": counted sequences with at least one hit (a deleted sample's included),
             "samples": [{"sample_name", "colour", "queries_hit", "kmers_found"}, ...]}
        `samples` leaves out deleted samples and samples no sequence hit; most sequences first, ties to the lowest colour; limit=N
        keeps the first N (cut on the host).  `seqs` is any iterable of ASCII sequences, fed in slices of about 8 x `batch_kmers`
        k-mers, as search_stream slices its input.  Multi-GPU (devices=[...]) indexes are refused."""
        from ..tally import record
        limit = check_limit(limit)
        self._check_stream_query(seqs, threshold)
        self._refuse_group("a query-set tally")
        k = int(self.kmer_size)
        with self._device_lock():
            t = self.storage.new_tally()
            try:
                for chunk in self._slices(iter(seqs), 64, None, batch_kmers * 8, k):
                    t.add(chunk, k, threshold)
                hit, found, totals = t.fetch()
            finally:
                t.close()
            excluded = self._excluded_colours()
        return record(hit, found, totals, self._name_of(), excluded, limit)

    # ------------------------------------------------------------------ read classification
    def _classify_groups(self, groups, others):
        """(group_of uint32[matrix columns], group names) of classify.classify_plan over this index's colours: a deleted sample, a
        colour without a metadata record and a column behind the metadata are in no group."""
        from ..classify import NONE, classify_plan
        names = []
        for c in range(self.num_samples):
            try:
                names.append(self.colour_to_sample(c))
            except KeyError:
                names.append(DELETION_SPECIAL_SAMPLE_NAME)
        group_of, group_names = classify_plan(names, groups, others)
        n_cols = int(self.storage.get_integer("number_of_cols"))
        full = np.full(n_cols, NONE, dtype=np.uint32)
        full[:min(n_cols, group_of.size)] = group_of[:n_cols]
        return full, group_names

    def classify_arrays(self, seqs, groups, threshold=1.0, others=None, batch_kmers=1 << 19):
        """The per-record question of a read set: which GROUP of samples does each sequence belong to -- answered on the device
        (bigsi_hip_classify_stream: per sequence and group the hits search(seq, threshold) reports are weighed behind the row-AND
        kernels; no hit list is built and 48 bytes per sequence leave the device).  Yields (chunk, records) per slice of the input:
        the slice's sequences and a structured array of classify.RECORD_DTYPE, one record each, whose group ids index the names
        classify.classify_plan(names, groups, others) gives.  `groups` is what collapse takes (a mapping group -> [samples] or (sample,
        group) pairs); `seqs` is any iterable of ASCII sequences, fed in slices of about 8 x `batch_kmers` k-mers, as tally slices its
        input.  Multi-GPU (devices=[...]) indexes are refused."""
        self._check_stream_query(seqs, threshold)
        from ..collapse import check_groups
        check_groups(groups)
        self._refuse_group("read classification")
        k = int(self.kmer_size)
        with self._device_lock():
            group_of, group_names = self._classify_groups(groups, others)
            for chunk in self._slices(iter(seqs), 64, None, batch_kmers * 8, k):
                for s in chunk:
                    if not isinstance(s, str) or not s.isascii():
                        raise ValueError("read classification takes ASCII sequences (queries with other characters are out of scope)")
                yield chunk, self.storage.classify(chunk, k, threshold, group_of, len(group_names))

    def classify(self, seqs, groups, threshold=1.0, margin=1, others=None):
        """classify_arrays over all of `seqs`, as names: {"groups": [group names in id order], "records": [one dict per sequence:
        "verdict" (assigned / ambiguous / unclassified / skipped), "group" (the assigned group), "best_sample" (the lowest sample of
        the best group that found most k-mers), "num_kmers", "min_kmers", "groups_hit", "samples_hit" and best_* / second_* with group
        names for ids], "summary": {"reads", "assigned": {group: reads}, "ambiguous", "unclassified", "skipped"}}.  The verdict rule is
        classify.verdicts': assigned when one group is hit or the best group found at least `margin` k-mers more than the next.  A
        colour the metadata has no record of is reported by its colour alone."""
        from ..classify import RECORD_DTYPE, result, verdicts
        verdicts(np.zeros(0, RECORD_DTYPE), [], margin)          # (the margin is checked before any device call)
        parts = [rec for _, rec in self.classify_arrays(seqs, groups, threshold, others)]
        records = np.concatenate(parts) if parts else np.zeros(0, RECORD_DTYPE)
        with self._device_lock():
            _, group_names = self._classify_groups(groups, others)
        return result(records, group_names, self._name_of(), margin)

    # ------------------------------------------------------------------ group association
    def _associate_groups(self, groups, others):
        """(group_of uint32[matrix columns], group names, sizes) of associate.associate_plan over this index's colours, placed as
        _classify_groups places its own: a deleted sample, a colour without a metadata record and a column behind the metadata are in
        no group."""
        from ..associate import associate_plan
        from ..classify import NONE
        names = []
        for c in range(self.num_samples):
            try:
                names.append(self.colour_to_sample(c))
            except KeyError:
                names.append(DELETION_SPECIAL_SAMPLE_NAME)
        group_of, group_names, _ = associate_plan(names, groups, others)
        n_cols = int(self.storage.get_integer("number_of_cols"))
        full = np.full(n_cols, NONE, dtype=np.uint32)
        full[:min(n_cols, group_of.size)] = group_of[:n_cols]
        sizes = np.bincount(full[full != NONE].astype(np.int64), minlength=len(group_names)).astype(np.int64)
        return full, group_names, sizes

    def associate_arrays(self, seqs, groups, threshold=1.0, others=None, batch_kmers=1 << 19):
        """The question of a GWAS or a marker screen: for every sequence (unitig, gene, probe), how many samples of each GROUP hold it
        -- answered on the device (bigsi_hip_associate_stream: the result vectors ANDed with one mask per group and popcounted behind
        the row-AND kernels; no hit list is built and n_groups + 4 integers per sequence leave the device).  Yields (slice, counts,
        info) per slice of the input: the slice's sequences, counts uint32[len(slice), n_groups] in the group order
        associate.associate_plan(names, groups, others) gives, and a structured array of associate.INFO_DTYPE.  `groups` is what
        collapse takes (a mapping group -> [samples] or (sample, group) pairs); `seqs` is any iterable of ASCII sequences, fed in
        slices of about 8 x `batch_kmers` k-mers, as classify slices its input.  Multi-GPU (devices=[...]) indexes are refused."""
        self._check_stream_query(seqs, threshold)
        from ..collapse import check_groups
        check_groups(groups)
        self._refuse_group("group association")
        k = int(self.kmer_size)
        with self._device_lock():
            group_of, group_names, _ = self._associate_groups(groups, others)
            for chunk in self._slices(iter(seqs), 64, None, batch_kmers * 8, k):
                for s in chunk:
                    if not isinstance(s, str) or not s.isascii():
                        raise ValueError("group association takes ASCII sequences (queries with other characters are out of scope)")
                counts, info = self.storage.associate(chunk, k, threshold, group_of, len(group_names))
                yield chunk, counts, info

    def associate(self, seqs, groups, threshold=1.0, others=None, min_af=None):
        """associate_arrays over all of `seqs`, as associate.result gives it: {"groups": [group names in id order], "sizes": the live
        samples of each, "total", "records": [per kept sequence "index", "num_kmers", "min_kmers", "samples_hit", "grouped_hit" and
        "groups": {name: "hit", "prevalence", "log2_odds", "chi2", "p" -- group against the rest of the grouped samples}], "dropped"}.
        min_af=F drops the sequences whose grouped hit fraction lies outside [F, 1 - F]."""
        from ..associate import INFO_DTYPE, result
        result(np.zeros((0, 1), np.uint32), np.zeros(0, INFO_DTYPE), ["x"], [0], min_af)          # (min_af is checked before any device call)
        parts = [(c, i) for _, c, i in self.associate_arrays(seqs, groups, threshold, others)]
        with self._device_lock():
            _, group_names, sizes = self._associate_groups(groups, others)
        counts = np.concatenate([c for c, _ in parts]) if parts else np.zeros((0, len(group_names)), np.uint32)
        info = np.concatenate([i for _, i in parts]) if parts else np.zeros(0, INFO_DTYPE)
        return result(counts, info, group_names, sizes, min_af)

    # ------------------------------------------------------------------ panel genotyping
    def genotype_arrays(self, probes, allele_of, n_variants, threshold=1.0, plane_bytes=1 << 30, planes=True):
        """Every sample's call for a panel of variants -- answered on the device (bigsi_hip_genotype: the probes' result vectors are
        ORed into one bit plane per allele behind the row-AND kernels, the calls and counts come from the planes by AND, AND-NOT and
        popcount; no hit list is built).  probes: ASCII sequences; allele_of[i]: 2 v + a (a = 0 ref, 1 alt) for probe i of variant
        v < n_variants, or genotype.NONE.  Returns (ref_planes, alt_planes: uint8[n_variants, ceil(num_cols / 8)] in the row format,
        or None with planes=False -- they are then never downloaded --, variant_counts uint32[n_variants, 4]: 0/0, 0/1, 1/1, missing,
        sample_counts uint32[num_cols, 2]: carried, called, allele_probes uint32[n_variants, 2]: the ref / alt probes with k-mers).
        Deleted samples are left out on the device: their bits are zero and they count nowhere.  The panel is cut by variant into
        slices whose planes fit `plane_bytes` of device memory, each with an accumulator of its own; a probe goes to its variant's
        slice only.  Multi-GPU (devices=[...]) indexes are refused."""
        from ..genotype import MAX_VARIANTS, NONE, slices
        self._check_stream_query(probes, threshold)
        probes = list(probes)
        allele_of = np.ascontiguousarray(allele_of, dtype=np.uint32).reshape(-1)
        n_variants = int(n_variants)
        if allele_of.size != len(probes):
            raise ValueError("allele_of has %d entries for %d probes" % (allele_of.size, len(probes)))
        if n_variants < 1:
            raise ValueError("n_variants must be >= 1, got %d" % n_variants)
        bad = np.flatnonzero((allele_of != NONE) & (allele_of.astype(np.int64) >= 2 * n_variants))
        if bad.size:
            raise ValueError("allele_of[%d] = %d is neither below 2 x n_variants (%d) nor NONE" % (bad[0], allele_of[bad[0]], 2 * n_variants))
        if int(plane_bytes) < 1:
            raise ValueError("plane_bytes must be >= 1, got %r" % (plane_bytes,))
        for s in probes:
            if not isinstance(s, str) or not s.isascii():
                raise ValueError("panel genotyping takes ASCII sequences (probes with other characters are out of scope)")
        self._refuse_group("panel genotyping")
        k = int(self.kmer_size)
        with self._device_lock():
            n_cols = int(self.storage.get_integer("number_of_cols"))
            rb = (n_cols + 7) // 8
            bits = np.ones(rb * 8, np.uint8)
            ex = self._excluded_colours()
            bits[ex[ex < n_cols]] = 0
            columns = np.packbits(bits)
            ref = np.zeros((n_variants, rb), np.uint8) if planes else None
            alt = np.zeros((n_variants, rb), np.uint8) if planes else None
            vc, sc, ap = np.zeros((n_variants, 4), np.uint32), np.zeros((n_cols, 2), np.uint32), np.zeros((n_variants, 2), np.uint32)
            for v0, v1, idx, rel in slices(allele_of, n_variants, rb, min(int(plane_bytes), 4 << 30)):
                if v1 - v0 > MAX_VARIANTS:
                    raise ValueError("a slice of %d variants: at most %d fit one accumulator (lower plane_bytes)" % (v1 - v0, MAX_VARIANTS))
                g = self.storage.new_genotype(v1 - v0, columns)
                try:
                    g.add([probes[i] for i in idx], k, threshold, rel)
                    r, a, vc[v0:v1], s, ap[v0:v1] = g.fetch(planes)
                finally:
                    g.close()
                sc += s
                if planes:
                    ref[v0:v1], alt[v0:v1] = r, a
        return ref, alt, vc, sc, ap

    def genotype_panel(self, panel, threshold=1.0, summary_only=False, plane_bytes=1 << 30):
        """genotype_arrays over a panel of probes -- concatenated `mykrobe variants make-probes` output: FASTA text, bytes or a path
        (genotype.parse_panel) -- as names: {"variants": [{"name", "ref_probes", "alt_probes", "counts": {"0/0", "0/1", "1/1", "./."},
        "calls": {sample_name: genotype, missing left out}}], "samples": [{"sample_name", "colour", "carried", "called"}]}; a variant
        one of whose alleles has no probe with k-mers is flagged "uncallable": True.  Deleted samples appear nowhere.
        summary_only=True leaves "calls" out, and the planes are then never downloaded."""
        from ..genotype import calls, parse_panel, result
        names, probes, allele_of = parse_panel(panel)
        if not names:
            raise ValueError("the panel holds no variant")
        ref, alt, vc, sc, ap = self.genotype_arrays(probes, allele_of, len(names), threshold, plane_bytes, planes=not summary_only)
        with self._device_lock():
            excluded = self._excluded_colours()
        matrix = None if summary_only else calls(ref, alt, sc.shape[0], excluded)
        return result(names, vc, sc, ap, self._name_of(), excluded, matrix)

    # ------------------------------------------------------------------ locus typing
    def typing_arrays(self, records, locus_of, n_loci, threshold=1.0, cell_bytes=1 << 30, cells=True, allele_of=None):
        """Each sample's best record per locus for a catalogue of allele records grouped into loci -- answered on the device
        (bigsi_hip_typing: a segmented max with argmax over the records' result vectors and counters behind the row-AND kernels; no
        hit list is built).  records: ASCII sequences; locus_of[i] < n_loci, or locus_typing.NONE; allele_of[i]: the record's
        identity (default: its position), ties go to the lowest.  Returns (best uint64[n_loci, num_cols] -- the key of
        include/bigsi_hip_typing.h, 0: no call; locus_typing.decode takes it apart --, hits uint32[n_loci, num_cols], or None, None
        with cells=False -- they are then never downloaded --, locus_counts uint32[n_loci, 3]: called, exact, multiple,
        sample_counts uint32[num_cols, 2]: called, exact, records uint32[n_loci]: the locus's records with k-mers).  Deleted
        samples are left out on the device: their cells are zero and they count nowhere.  The scheme is cut by locus into slices
        whose cells fit `cell_bytes` of device memory, each with an accumulator of its own; a record goes to its locus's slice only.
        Multi-GPU (devices=[...]) indexes are refused."""
        from ..locus_typing import MAX_ALLELE, MAX_LOCI, NONE, slices
        self._check_stream_query(records, threshold)
        records = list(records)
        locus_of = np.ascontiguousarray(locus_of, dtype=np.uint32).reshape(-1)
        allele_of = np.arange(len(records), dtype=np.uint32) if allele_of is None else np.ascontiguousarray(allele_of, dtype=np.uint32).reshape(-1)
        n_loci = int(n_loci)
        if locus_of.size != len(records) or allele_of.size != len(records):
            raise ValueError("locus_of and allele_of have %d and %d entries for %d records" % (locus_of.size, allele_of.size, len(records)))
        if n_loci < 1:
            raise ValueError("n_loci must be >= 1, got %d" % n_loci)
        bad = np.flatnonzero((locus_of != NONE) & (locus_of.astype(np.int64) >= n_loci))
        if bad.size:
            raise ValueError("locus_of[%d] = %d is neither below n_loci (%d) nor NONE" % (bad[0], locus_of[bad[0]], n_loci))
        bad = np.flatnonzero((locus_of != NONE) & (allele_of > MAX_ALLELE))
        if bad.size:
            raise ValueError("allele_of[%d] = %d is above %d" % (bad[0], allele_of[bad[0]], MAX_ALLELE))
        if int(cell_bytes) < 1:
            raise ValueError("cell_bytes must be >= 1, got %r" % (cell_bytes,))
        for s in records:
            if not isinstance(s, str) or not s.isascii():
                raise ValueError("locus typing takes ASCII sequences (records with other characters are out of scope)")
        self._refuse_group("locus typing")
        k = int(self.kmer_size)
        with self._device_lock():
            n_cols = int(self.storage.get_integer("number_of_cols"))
            bits = np.ones((n_cols + 7) // 8 * 8, np.uint8)
            ex = self._excluded_colours()
            bits[ex[ex < n_cols]] = 0
            columns = np.packbits(bits)
            best = np.zeros((n_loci, n_cols), np.uint64) if cells else None
            hits = np.zeros((n_loci, n_cols), np.uint32) if cells else None
            lc, sc, rec = np.zeros((n_loci, 3), np.uint32), np.zeros((n_cols, 2), np.uint32), np.zeros(n_loci, np.uint32)
            for l0, l1, idx, rel in slices(locus_of, n_loci, n_cols, min(int(cell_bytes), 4 << 30)):
                if l1 - l0 > MAX_LOCI:
                    raise ValueError("a slice of %d loci: at most %d fit one accumulator (lower cell_bytes)" % (l1 - l0, MAX_LOCI))
                t = self.storage.new_typing(l1 - l0, columns)
                try:
                    t.add([records[i] for i in idx], k, threshold, rel, allele_of[idx])
                    b, h, lc[l0:l1], s, rec[l0:l1] = t.fetch(cells)
                finally:
                    t.close()
                sc += s
                if cells:
                    best[l0:l1], hits[l0:l1] = b, h
        return best, hits, lc, sc, rec

    def type_samples(self, scheme, threshold=1.0, profiles=None, summary_only=False, loci_map=None, cell_bytes=1 << 30):
        """typing_arrays over a scheme of allele records -- FASTA text, bytes or a path, PubMLST-style names locus_allele or a
        record<TAB>locus loci_map (locus_typing.parse_scheme) -- as names: {"loci": [{"name", "records", "called", "exact",
        "multiple"}], "samples": [{"sample_name", "colour", "called", "exact", "ST" (with profiles: a PubMLST profiles table; the
        matching row's ST when every locus is exact, "novel" when none matches, "-" otherwise), "calls": {locus: {"allele",
        "fraction", "exact", "n_hits"}, loci without a call left out}}]}.  Deleted samples appear nowhere.  summary_only=True leaves
        "calls" and "ST" out, and the cells are then never downloaded."""
        from ..locus_typing import calls, parse_profiles, parse_scheme, result
        loci, _, alleles, records, locus_of, allele_of = parse_scheme(scheme, loci_map)
        if not loci:
            raise ValueError("the scheme holds no record")
        table = parse_profiles(profiles, loci) if profiles is not None else None
        best, hits, lc, sc, rec = self.typing_arrays(records, locus_of, len(loci), threshold, cell_bytes, cells=not summary_only, allele_of=allele_of)
        with self._device_lock():
            excluded = self._excluded_colours()
        matrix = None if summary_only else calls(best, alleles, hits)
        return result(loci, lc, sc, rec, self._name_of(), excluded, matrix, table)

    # ------------------------------------------------------------------ column compaction: vacuum / extract
    def _colour_names(self):
        """names[c] of every colour, DELETION_SPECIAL_SAMPLE_NAME for a deleted one; the matrix must be as wide as the metadata."""
        n = self.num_samples
        cols = int(self.storage.get_integer("number_of_cols"))
        if cols != n:
            raise ValueError("the matrix has %d columns and the metadata %d colours" % (cols, n))
        return [self.colour_to_sample(c) for c in range(n)]

    def vacuum(self, shrink=True):
        """Remove the columns of deleted samples from the matrix (bigsi_hip_compact_columns, in place on the device) and renumber
        the samples that stay 0 .. K-1 in their old order: afterwards the index is the one BIGSI.build makes from the kept samples'
        filters in colour order -- rows, metadata records, search results and scores (which depend on the number of samples).
        The names of the removed samples can be inserted again.  shrink: also give the freed row stride back
        (bigsi_hip_shrink_to_fit).  Returns the number of columns removed; 0, without touching the device, when nothing is deleted.
        The matrix is compacted first and the metadata rewritten after it, in this process's memory; nothing is on disk before the
        caller's sync().  A process that dies in between loses nothing -- its snapshot is the index before the vacuum -- but an
        exception between the two steps (none is expected: the second is dictionary writes) would leave THIS object's metadata
        naming the old colours: drop the resident index and open the snapshot again."""
        from ..compact import vacuum_plan
        from .metadata import _COUNT, _k
        if not isinstance(shrink, bool):
            raise TypeError("shrink must be a bool, got %r" % (shrink,))
        with self._device_lock():
            names = self._colour_names()
            keep, kept = vacuum_plan(names)
            removed = len(names) - len(kept)
            if removed == 0:
                return 0
            st = self.storage
            if st.compact_columns(keep) != len(kept):
                raise RuntimeError("the device kept another number of columns than the metadata names")
            for j, name in enumerate(kept):
                st.set_integer(_k(name), j)
                st.set_string(_k(j), name)
            st.delete_records([st.convert_to_string_key(_k(c)) for c in range(len(kept), len(names))])
            # the tombstones of delete_sample: "<name>:int" = -1
            st.delete_records([key for key in st.record_keys(_k("")) if key.endswith(":int") and key != st.convert_to_integer_key(_k(_COUNT))
                               and st[key] == b"-1"])
            st.set_integer(_k(_COUNT), len(kept))
            self.bitmatrix.set_num_cols(len(kept))
            for batch in self.__dict__.pop("_workspaces", {}).values():
                batch.close()
            self._metadata_changed()
            self.scorer = Scorer(self.num_samples)
            if shrink:
                st.shrink_to_fit()
            return removed

    def extract(self, config, samples):
        """A new index under `config` (same m, h, k, same device; nothing stored under it yet) that holds the named samples of
        this one, in THIS index's colour order (bigsi_hip_extract_columns: device to device, this index is only read) -- the index
        BIGSI.build makes from those samples' filters.  A subset that is searched again and again is extracted once and then costs
        |subset| / N of the bytes per query.  KeyError for a name that is unknown or deleted, ValueError for an empty list or a
        name given twice.  Returns the new BIGSI."""
        from ..compact import extract_plan
        if isinstance(samples, (str, bytes)):
            raise TypeError("samples must be a list of sample names, got %r" % type(samples))
        samples = list(samples)
        if not samples or len(set(samples)) != len(samples):
            extract_plan([], samples)                   # (raises the ValueError, before anything is read)
        self._refuse_group("column extraction")
        with self._device_lock():
            keep, picked = extract_plan(self._colour_names(), samples)

            def fill(storage):
                if storage.extract_columns_from(self.storage, keep) != len(picked):
                    raise RuntimeError("the device extracted another number of columns than the metadata names")
                SampleMetadata(storage).add_samples(picked)
            return self._derive(config, self.bloomfilter_size, fill)

    # ------------------------------------------------------------------ column collapse: groups of samples ORed into one column each
    def collapse(self, config, groups, keep_others=False):
        """A new index under `config` (same m, h, k, same device; a storage-config name of its own, nothing stored under it yet) in
        which every GROUP of samples of this one is one column: the OR of its members' columns (bigsi_hip_collapse_columns_into:
        device to device, this index is only read).  The Bloom filter of a union of k-mer sets is the OR of the members' filters, so
        the new index is bit for bit the one BIGSI.build makes from the OR-ed filters under the group names, and every exact hit of
        a member is a hit of its group: the small index that is searched first, at |groups| / N of the bytes per query.
        groups: an ordered mapping group name -> [sample names], or (sample, group) pairs; the new colours follow the order of a
        group's first appearance, so singleton groups REORDER samples.  Deleted samples are dropped; unlisted samples are dropped, or
        with keep_others each stays as a group of its own under its own name, after the named groups.  KeyError / ValueError as
        collapse.collapse_plan says (which also gives the membership: collapse_plan(names, groups, keep_others)[2]).  Returns the
        new BIGSI."""
        from ..collapse import check_groups, collapse_plan
        check_groups(groups, keep_others)               # (whatever it raises, it raises before anything is read)
        self._refuse_group("column collapse")
        with self._device_lock():
            group_of, group_names, _ = collapse_plan(self._colour_names(), groups, keep_others)

            def fill(storage):
                if self.storage.collapse_columns_into(storage, group_of, len(group_names)) != len(group_names):
                    raise RuntimeError("the device made another number of columns than there are groups")
                SampleMetadata(storage).add_samples(group_names)
            return self._derive(config, self.bloomfilter_size, fill)

    # ------------------------------------------------------------------ consensus collapse: the core of every group of samples
    def consensus(self, config, groups, percent=100, keep_others=False):
        """A new index under `config` (as for collapse: same m, h, k, same device, a storage-config name of its own, nothing stored
        under it yet) in which every GROUP of samples of this one is one column that keeps a bit only where at least `percent` % of
        the group's members have it (bigsi_hip_consensus_columns_into: device to device, this index is only read): the CORE of the
        group where collapse keeps its union.  need = max(1, ceil(percent x size / 100)) members (consensus.need_of, integers only).
        A k-mer that at least `need` members hold has every one of its h bits in at least `need` member columns, so it is still found
        in the group's column -- no false negatives for the core --, and the column's fill, hence its false-positive rate, falls as
        percent rises where an OR of many members saturates.  percent=100 is bit for bit the index BIGSI.build makes from the AND of
        the members' filters under the group names; percent=1 is collapse() for groups of up to 100 members.  groups, keep_others,
        the colour order and KeyError / ValueError as for collapse (collapse.collapse_plan); a sample that keep_others keeps on its
        own is a group of one, needs 1 and is copied.  percent: an int in [1, 100] (TypeError for a bool or a float, ValueError out
        of range).  Returns the new BIGSI."""
        from ..collapse import check_groups, collapse_plan
        from ..consensus import check_percent, group_sizes, need_of
        check_groups(groups, keep_others)               # (whatever these two raise, they raise before anything is read)
        percent = check_percent(percent)
        self._refuse_group("consensus collapse")
        with self._device_lock():
            group_of, group_names, _ = collapse_plan(self._colour_names(), groups, keep_others)
            need = need_of(group_sizes(group_of, len(group_names)), percent)

            def fill(storage):
                if self.storage.consensus_columns_into(storage, group_of, len(group_names), need) != len(group_names):
                    raise RuntimeError("the device made another number of columns than there are groups")
                SampleMetadata(storage).add_samples(group_names)
            return self._derive(config, self.bloomfilter_size, fill)

    # ------------------------------------------------------------------ what extract, collapse, consensus and fold_into share
    def _refuse_group(self, what):
        if self.storage.res.is_group:
            from .._lib import ERR_STATE, BigsiHipError
            raise BigsiHipError(ERR_STATE, "%s is not available for multi-GPU (devices=[...]) indexes" % what)

    def _check_derived_config(self, config, new_m):
        for key, want in (("m", new_m), ("h", self.num_hashes), ("k", self.kmer_size)):
            if int(config[key]) != int(want):
                raise ValueError("the new index must have %s = %d, its config says %d" % (key, want, config[key]))

    def _derive(self, config, new_m, fill):
        """The index under `config` (m = new_m, this index's h and k, a storage-config name of its own, nothing stored under it yet)
        made from this one by fill(storage): the device call into the opened, empty storage and the sample metadata that goes with
        it.  On any failure the new storage is emptied again.  Returns the new BIGSI."""
        from .index import BLOOMFILTER_SIZE_KEY, NUM_HASH_FUNCTS_KEY
        self._check_derived_config(config, new_m)
        with self._device_lock():
            storage = get_storage(config)
            if storage.res is self.storage.res:
                raise ValueError("the new index needs a storage-config name of its own")
            if SampleMetadata(storage).num_samples or int(storage.get("number_of_cols:int", b"0")):
                raise ValueError("the index described by the new config is not empty")
            try:
                storage.set_integer(BLOOMFILTER_SIZE_KEY, int(new_m))
                storage.set_integer(NUM_HASH_FUNCTS_KEY, int(self.num_hashes))
                storage.set_integer("number_of_rows", int(new_m))
                storage.set_integer("number_of_cols", 0)
                storage.res.ensure_open()
                fill(storage)
                storage.sync()
            except BaseException:
                storage.delete_all()          # (it was empty when we came: nothing half-made stays resident under the new name)
                raise
            storage.close()
        return type(self)(config)

    # ------------------------------------------------------------------ row folding: the same index under a smaller Bloom filter
    def fold(self, factor, trim=True):
        """Fold the index in place to m' = m / factor rows (bigsi_hip_fold_rows: row r becomes the OR of the rows r, r + m', ...,
        r + (factor - 1) m').  Because a k-mer's row is floor_mod(hash, m) and m' divides m, the result is bit for bit the index
        BIGSI.build makes from the same samples under a config with m = m': rows, search results, counts and scores; no false
        negative appears, the false-positive rate rises (sample_stats() of the folded index says to what; fold.fold_estimate
        predicts it).  The stored bloomfilter_size and number_of_rows follow; from now on the index is described by a config with
        m = m'.  trim: also give the freed rows back (bigsi_hip_trim_rows) -- that needs room for the smaller copy beside the
        matrix, and a trim that finds none leaves the allocation as it is and reports trimmed: False.  Nothing is on disk before
        the caller's sync().  Returns {"m": m', "factor": factor, "trimmed": bool}."""
        from .._lib import ERR_NOMEM, BigsiHipError
        from ..fold import fold_plan
        from .index import BLOOMFILTER_SIZE_KEY
        if not isinstance(trim, bool):
            raise TypeError("trim must be a bool, got %r" % (trim,))
        new_m = fold_plan(int(self.bloomfilter_size), factor)
        self._refuse_group("row folding")
        with self._device_lock():
            st = self.storage
            trimmed = False
            if factor > 1:
                for batch in self.__dict__.pop("_workspaces", {}).values():
                    batch.close()
                if st.fold_rows(factor) != new_m:
                    raise RuntimeError("the device folded to another number of rows than the host worked out")
                st.set_integer(BLOOMFILTER_SIZE_KEY, new_m)
                st.set_integer("number_of_rows", new_m)
                self.bloomfilter_size = new_m
                self.bitmatrix._rows = new_m
                if isinstance(self.config, dict) and "m" in self.config:
                    self.config = dict(self.config, m=new_m)
                self._metadata_changed()
                if trim:
                    try:
                        st.trim_rows()
                        trimmed = True
                    except BigsiHipError as e:
                        if e.code != ERR_NOMEM:
                            raise
            return {"m": new_m, "factor": int(factor), "trimmed": trimmed}

    def fold_into(self, config, factor):
        """A new index under `config` (m = this index's m / factor, same h and k, same device, a storage-config name of its own,
        nothing stored under it yet) that holds this index folded by `factor` (bigsi_hip_fold_rows_into: device to device, this
        index is only read) -- the index BIGSI.build makes from the same samples under `config`.  The sample metadata is copied
        unchanged: same colours, and deleted samples stay deleted.  On any failure the new storage is emptied again.  Returns the
        new BIGSI."""
        from ..fold import fold_plan
        from .metadata import _k
        new_m = fold_plan(int(self.bloomfilter_size), factor)
        self._check_derived_config(config, new_m)          # (a config that does not fit is a bad argument: said before the storage is looked at)
        self._refuse_group("row folding")

        def fill(storage):
            mine = self.storage
            if storage.fold_rows_from(mine) != int(mine.get_integer("number_of_cols")):
                raise RuntimeError("the device folded another number of columns than the index holds")
            for key in mine.record_keys(_k("")):          # colours, names and the tombstones of deleted samples, as they are
                storage[key] = mine[key]
        return self._derive(config, new_m, fill)

    def _device_lock(self):
        import threading
        return self.storage.res.__dict__.setdefault("_lock", threading.RLock())

    def _names_of(self, cols, exact):
        """names[c] for the C++ assembly of result dicts: the sample name of every colour that occurs in `cols` (looked up once),
        None for a deleted sample (its hits are dropped).  Returns None instead when a colour has no name (beyond num_samples on the
        exact route, or below it with no metadata record): a KeyError in the reference, which the Python loop raises at the right place."""
        ns = self.num_samples
        names = [None] * ns
        for c in np.unique(cols).tolist():
            if c < ns:
                try:
                    name = self.colour_to_sample(c)
                except KeyError:          # a colour below num_samples without a name: the per-record Python loop raises it when its turn comes
                    return None
                names[c] = None if name == DELETION_SPECIAL_SAMPLE_NAME else name
            elif exact:
                return None
        return names

    def _emit_native(self, res, nk, nu, off64, n_hits, colours, counts, threshold, score):
        """_emit's loop in the C++ extension (bigsi_amd/_results.cpp): the same dicts, built from the arrays without a Python
        statement per hit.  What stays here: the reference's errors (raised when the offending sequence's turn comes), the sample
        names of the colours that occur (looked up once per slice), the closed-form score columns (numpy, all hits at once)."""
        _, chunk, payload = res
        exact = threshold == 1.0
        ns = self.num_samples
        # where the reference raises: a query without k-mers (either branch); score=True on a one-k-mer query that has hits
        bad = nu == 0
        if score:
            bad = bad | ((nk == 1) & (n_hits > 0))
        stop = int(np.argmax(bad)) if bad.any() else len(chunk)
        total = int(off64[stop])
        cols = np.ascontiguousarray(colours[:total])
        names = self._names_of(cols, exact)
        if names is None:
            yield from self._emit(res, threshold, score, native=False)
            return
        scored = (payload[7][:total], payload[5], payload[6]) if score else None
        # (blocks of sequences: the consumer gets its first results before the whole slice is assembled)
        yield from zip(chunk[:stop], native_result_lists(nk[:stop], nu[:stop], off64[:stop + 1], cols, counts, exact, names, scored, self.scorer.DB_SIZE))
        if stop < len(chunk):
            if nu[stop] == 0:
                if exact:
                    raise TypeError("reduce() of empty sequence with no initial value")
                raise UnboundLocalError("local variable 'cumsum' referenced before assignment")
            raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")

    def _emit(self, res, threshold, score, native=True):
        """(sequence, results) pairs of one slice from what the worker left: the reference's errors in stream order.  Plain Python
        over lists made once per slice (a numpy call per sequence costs more than the few hits a read has)."""
        from ..scoring import SCORE_KEYS
        kind, chunk, payload = res
        if kind == "error":
            raise payload
        if kind == "done":
            yield from zip(chunk, payload)
            return
        nk, nu, off, colours, counts = payload[:5]
        exact = threshold == 1.0
        off64 = off.astype(np.int64)
        n_hits = np.diff(off64)
        special = np.flatnonzero((n_hits > 0) | (nu == 0)).tolist()
        if not special:
            for s in chunk:
                yield s, []
            return
        if _results is not None and native:
            yield from self._emit_native(res, nk, nu, off64, n_hits, colours, counts, threshold, score)
            return
        scored = None
        if score and int(off64[-1]):
            # the scored rows (closed-form fields, presence strings) of a slice are made 256 hits at a time, as they are needed: 4096
            # hits of 970 positions at once are 4 MB of fresh strings per slice -- page faults and cache misses made that 7 us per hit
            # where blocks that stay in the cache take 4
            bits, boff, rec = payload[5:8]
            lengths, db, blk = np.repeat(nk.astype(np.int64), n_hits), self.scorer.DB_SIZE, {"lo": 0, "rows": []}

            class _Blocks(object):
                def __getitem__(self_, t):
                    lo = blk["lo"]
                    if not lo <= t < lo + len(blk["rows"]):
                        lo = t - t % 256
                        hi = min(lo + 256, len(lengths))
                        b0 = int(boff[lo])
                        blk["rows"] = scored_rows(rec[lo:hi], bits[b0:int(boff[hi])], boff[lo:hi + 1] - boff[lo], lengths[lo:hi], db)
                        blk["lo"] = lo
                    return blk["rows"][t - lo]
            scored = _Blocks()
        offs, nus, nks, cols, cnts = off64.tolist(), nu.tolist(), nk.tolist(), colours.tolist(), counts.tolist()
        ns, name_of, deleted = self.num_samples, self.colour_to_sample, DELETION_SPECIAL_SAMPLE_NAME
        names = {}
        keys = ("percent_kmers_found", "num_kmers", "num_kmers_found", "sample_name") + SCORE_KEYS + ("kmer-presence",)
        prev = 0
        for i in special:
            for s in chunk[prev:i]:
                yield s, []
            prev = i + 1
            u = nus[i]
            if u == 0:
                # the reference fails on a query without k-mers: reduce() over nothing on the exact branch
                # (utils/fncts.py:24-25), an unbound accumulator on the other (graph/bigsi.py:35-44)
                if exact:
                    raise TypeError("reduce() of empty sequence with no initial value")
                raise UnboundLocalError("local variable 'cumsum' referenced before assignment")
            if score and nks[i] == 1:
                # the reference builds a 1-D matrix from a single row and then indexes it with two subscripts
                raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
            lo, hi = offs[i], offs[i + 1]
            if exact:
                # exact_filter (graph/bigsi.py:192-205): every set bit, ascending; a colour without a name is a KeyError
                order = range(lo, hi)
            else:
                # inexact_filter (:211-230): only colours < num_samples are zipped in; stable sort by count, descending
                order = sorted((t for t in range(lo, hi) if cols[t] < ns), key=lambda t: -cnts[t])
            out = []
            for t in order:
                c = cols[t]
                name = names.get(c)
                if name is None:
                    name = names[c] = name_of(c)
                if name == deleted:
                    continue
                f = u if exact else cnts[t]
                if scored is None:
                    out.append({"percent_kmers_found": round(100 * float(f) / u, 2), "num_kmers": u, "num_kmers_found": f, "sample_name": name})
                else:
                    pct, fields, text = scored[t]
                    out.append(dict(zip(keys, (pct, u, f, name) + fields + (text,))))
            yield chunk[i], out
        for s in chunk[prev:]:
            yield s, []

    def _search_stream_batches(self, seqs, threshold=1.0, score=False, batch_size=None, batch_kmers=1 << 19, limit=None):
        """search_stream over this object's own batch workspaces (what a multi-GPU index uses), two workspaces deep: while
        the GPU runs batch i+1 the host fetches and assembles batch i (fetches wait on the batch's own completion event, not
        on the stream).  A device batch closes after `batch_size` sequences if given, else once it holds about
        `batch_kmers` k-mers (about 540 x 1 kbp, or ~17000 reads of 61 bp: 4 ms of device work on a 125 GB index, enough to hide the
        per-batch host work; measured 117 M lookups/s with 2^18 and 124 M with 2^19 k-mers per batch at C3)."""
        assert threshold <= 1
        k, ws = self.kmer_size, {}

        def submit(chunk, slot):
            try:
                plain = "".join(chunk).isascii()           # one pass at C speed
            except TypeError:                             # (bytes among the sequences)
                plain = all(s.isascii() for s in chunk)
            if not plain or self._limit_fallback(chunk, score, limit):      # rare: answered at once through search_batch
                return [_Done(self.search_batch(chunk, threshold, score, limit=limit)), chunk]
            batch = self._workspace(slot, chunk, ws)
            self._set_limit(batch, limit)
            self._launch(batch, threshold)
            return [batch, chunk]

        def begin(p):
            # score=True, three batches deep: the scored hits of the batch launched one step ago are only QUEUED here (K5 + K6 beside
            # the batch just launched); done() picks them up a step later.  The reference's errors for degenerate queries are
            # raised from here: kept for done(), so that they surface in stream order (after the results of the batch before)
            if not isinstance(p[0], _Done):
                try:
                    p.append(self._collect_begin(p[0], len(p[1]), threshold, score, deferred=True))
                except Exception as e:  # noqa: BLE001
                    p.append(e)

        def done(p):
            if isinstance(p[0], _Done):
                return p[0].results
            if len(p) > 2 and isinstance(p[2], Exception):
                raise p[2]
            return self._collect_end(p[2]) if len(p) > 2 else self._collect(p[0], len(p[1]), threshold, score)

        # sequences are taken from the iterable in slices (C speed: millions of reads go through here); without a
        # batch_size the slice length follows the k-mers per sequence seen so far, so that a batch holds ~batch_kmers of them
        it = iter(seqs)
        take = batch_size if batch_size else 64
        try:
            yield from self._stream_loop(it, take, batch_size, batch_kmers, k, submit, done, begin if score else None, 3 if score else 2)
        finally:
            for b_ in ws.values():
                b_.close()

    @staticmethod
    def _slices(it, take, batch_size, batch_kmers, k):
        """Cut an iterable of sequences into lists: `batch_size` sequences each if given, else about `batch_kmers` k-mers -- the slice
        length follows the k-mers per sequence seen so far, and a slice that overshoots (reads first, genomes later) is cut at the
        sequence that reaches the target, the rest held back for the next slice (a plain list: nothing is wrapped around the iterator)."""
        from itertools import islice
        held_back = []

        def pull(n):
            out = held_back[:n]
            del held_back[:n]
            if len(out) < n:
                out += list(islice(it, n - len(out)))
            return out

        while True:
            chunk = pull(take)
            if not chunk:
                return
            if not batch_size:
                held = sum(map(len, chunk)) - (k - 1) * len(chunk)
                while held < batch_kmers:                # top the slice up to a full batch
                    per = max(held // len(chunk), 1)
                    more = pull(max((batch_kmers - held + per - 1) // per, 1))
                    if not more:
                        break
                    chunk += more
                    held = sum(map(len, chunk)) - (k - 1) * len(chunk)
                    held = max(held, len(chunk))
                if held > batch_kmers and len(chunk) > 1:
                    csum = np.cumsum(np.maximum(np.fromiter(map(len, chunk), dtype=np.int64, count=len(chunk)) - (k - 1), 1))
                    cut = int(np.searchsorted(csum, batch_kmers, side="left")) + 1
                    if cut < len(chunk):
                        held_back[:0] = chunk[cut:]
                        chunk = chunk[:cut]
                take = len(chunk)
            yield chunk

    @staticmethod
    def _stream_loop(it, take, batch_size, batch_kmers, k, submit, done, begin=None, depth=2):
        """submit(chunk, slot) launches a batch on workspace `slot` (of `depth`) and returns its handle; `depth` - 1 batches later
        done(handle) yields its results.  With `begin`, begin(handle) is called once the NEXT batch has been launched (the middle
        stage of a pipeline three deep: work queued beside that batch, collected by done() a step later)."""
        flight, slot = [], 0
        for chunk in BIGSI._slices(it, take, batch_size, batch_kmers, k):
            if len(flight) == depth:                     # the workspace about to be reused: its results first
                p = flight.pop(0)
                yield from zip(p[1], done(p))
            nxt = submit(chunk, slot)
            slot = (slot + 1) % depth
            if begin is not None and flight:
                begin(flight[-1])
            flight.append(nxt)
            if len(flight) == depth:
                p = flight.pop(0)
                yield from zip(p[1], done(p))
        if begin is not None and flight:
            begin(flight[-1])
        for p in flight:
            yield from zip(p[1], done(p))

    def lookup(self, kmers, remove_trailing_zeros=True):
        with self._device_lock():
            return KmerSignatureIndex.lookup(self, kmers, remove_trailing_zeros)

    def search_stream_arrays(self, seqs, threshold=1.0, batch_size=1 << 15):
        """The device's own answer, batch by batch, for callers to whom a Python dict per hit is too slow (millions of reads):
        yields (chunk, num_unique, hit_offsets, colours, counts) -- the sequences of the batch, their unique k-mer counts
        (uint32[n]), and its hit lists: sequence i matched colours[hit_offsets[i]:hit_offsets[i+1]] with that many of its
        k-mers (ascending colour; every colour < num_samples, deleted samples included: map names with colour_to_sample).
        Same two-deep pipeline as search_stream; ASCII sequences only (ValueError otherwise).  Not part of the reference's API."""
        assert threshold <= 1
        from itertools import islice
        it, pending, slot, ws = iter(seqs), None, 0, {}

        def finish(p):
            batch, chunk = p
            _, nu, _ = batch.unique()
            off, colours, counts = batch.hits()
            keep = colours < self.num_samples            # (columns beyond the last sample exist only as padding)
            if not keep.all():
                csum = np.concatenate([[0], np.cumsum(keep)])
                off, colours, counts = csum[off.astype(np.int64)].astype(np.uint64), colours[keep], counts[keep]
            return chunk, nu[:len(chunk)].copy(), off, colours, counts

        try:
            while True:
                chunk = list(islice(it, batch_size))
                if not chunk:
                    break
                batch = self._workspace(slot, chunk, ws)
                self._launch(batch, threshold)
                if pending is not None:
                    yield finish(pending)
                pending, slot = (batch, chunk), slot ^ 1
            if pending is not None:
                yield finish(pending)
        finally:
            for b_ in ws.values():
                b_.close()

    def _assemble(self, first_hit, colours, counts, u, exact, scored):
        """Result dicts of one sequence from its slice of the batch's hit lists; `scored` (score=True) = _score_hits' per-hit
        tuples, indexed by position in the hit lists, `first_hit` = position of this slice's first hit."""
        from ..scoring import SCORE_KEYS
        idx = np.arange(len(colours))
        if exact:
            # exact_filter (graph/bigsi.py:192-205): every set bit, ascending; a colour without a name is a KeyError
            order = idx
            found = [u] * len(colours)
        else:
            # inexact_filter (:211-230): only colours < num_samples are zipped in; stable sort by count, descending
            keep = colours < self.num_samples
            colours, counts, idx = colours[keep], counts[keep], idx[keep]
            order = np.argsort(-counts.astype(np.int64), kind="stable")
            colours, idx = colours[order], idx[order]
            found = counts[order].tolist()
        names = [self.colour_to_sample(c) for c in colours.tolist()]
        if scored is None:
            results = [BigsiQueryResult(0, name, f, u) for name, f in zip(names, found)]
            return [r.todict() for r in results if r.sample_name != DELETION_SPECIAL_SAMPLE_NAME]
        # BigsiQueryResult.todict (graph/bigsi.py:105-114) + add_score, written out: percent and scores come from the device
        keys = ("percent_kmers_found", "num_kmers", "num_kmers_found", "sample_name") + SCORE_KEYS + ("kmer-presence",)
        out = []
        for name, f, t in zip(names, found, idx.tolist()):
            if name == DELETION_SPECIAL_SAMPLE_NAME:
                continue
            pct, fields, col = scored[first_hit + t]
            out.append(dict(zip(keys, (pct, u, f, name) + fields + (col,))))
        return out
