"""Exact k-mer counting: Bloom filters from raw reads, with the k-mers seen fewer than C times left out.

`KmerCounter` is one shape over two libraries: "hip" is the device counter of libbigsi_hip.so (include/bigsi_hip_kmercount.h: a hash
table in HBM, counted, swept and hashed by kernels), "cpu" the host twin in the CPU library (the same eight entry points under that
library's prefix: the definition, a std::map), for hosts without a GPU.  Which one runs is the caller's explicit choice and never changes
behind their back: a missing library or device is an error, not a fall-back, and the hip-hbm backend never asks for the twin.  The
semantics are the SEMANTICS block of the twin's header; tests/kmercount_ref.py restates them in Python."""
import ctypes as C
import gzip
import os

import numpy as np

from . import _lib
from .bitrow import BitRow

MAX_K = 32
SLICE_BYTES = 64 << 20          # text read from a file at a time (cut back to whole records)
LIBRARIES = ("hip", "cpu")
_NAMES = ("create", "destroy", "reset", "add", "info", "spectrum", "fetch", "bloom")
_loaded = {}


def library_path(library):
    """Where the in-tree build of a library lies: libbigsi_<library>.so beside this file (the device library: _lib.LIB_PATH)."""
    return _lib.LIB_PATH if library == "hip" else os.path.join(os.path.dirname(os.path.abspath(__file__)), "libbigsi_%s.so" % library)


def load_library(library):
    """The loaded library with bigsi_<library>_kmer_counter_* and bigsi_<library>_last_error bound; raises when it has not been built."""
    if library not in LIBRARIES:
        raise ValueError("library must be 'hip' or 'cpu', got %r" % (library,))
    if library == "hip":
        return _lib.lib()
    if library not in _loaded:
        path = library_path(library)
        if not os.path.exists(path):
            raise _lib.BigsiHipError(_lib.ERR_STATE, "%s is missing: build it with bigsi_amd/%s/build.sh" % (path, library))
        L = C.CDLL(path)
        getattr(L, "bigsi_%s_last_error" % library).restype = C.c_char_p
        for name in _NAMES:
            res, args = _lib.KMERCOUNT_SIGNATURES["bigsi_hip_kmer_counter_" + name]
            fn = getattr(L, "bigsi_%s_kmer_counter_%s" % (library, name))
            fn.restype, fn.argtypes = res, args
        _loaded[library] = L
    return _loaded[library]


def check_k(k):
    """The counter's k, or ValueError: a key is one 64-bit word."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError("k must be an integer")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError("the k-mer counter takes k in [1, %d], got %d (a Bloom filter of longer k-mers is made from a k-mer list)" % (MAX_K, int(k)))
    return int(k)


def check_min_count(min_count):
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)):
        raise TypeError("min_count must be an integer")
    if not 1 <= int(min_count) <= 0xFFFFFFFF:
        raise ValueError("min_count must be in [1, 2^32 - 1], got %d" % int(min_count))
    return int(min_count)


def record_cut(text, fastq, last):
    """How many bytes of `text` are whole records (everything when `last`): a FASTA text is cut before its last header line, a FASTQ
    text of four-line records after a multiple of four lines."""
    if last:
        return len(text)
    if not fastq:
        at = max(text.rfind(b"\n>"), text.rfind(b"\r>"))
        return at + 1 if at >= 0 else 0
    # lines end in LF (CR LF included) or, in a text without any LF, in CR: count them, then walk back over the 0 to 3 lines of the
    # record the slice ends in -- a handful of searches whatever the slice size
    nl = b"\n" if b"\n" in text else b"\r"
    at = len(text)
    for _ in range(text.count(nl) % 4 + 1):
        at = text.rfind(nl, 0, at)
    return at + 1


class KmerCounter(object):
    """with KmerCounter(31) as c: c.add_file("reads.fastq.gz"); row = c.bloom(m, h, min_count=2)"""

    def __init__(self, k, expected_distinct=0, device=0, library="hip"):
        self.k = check_k(k)
        self.library, self._h = library, None
        self._L = load_library(library)
        h = C.c_void_p()
        self._check(self._fn("create")(int(device), self.k, int(expected_distinct), C.byref(h)))
        self._h = h

    def _fn(self, name):
        return getattr(self._L, "bigsi_%s_kmer_counter_%s" % (self.library, name))

    def _check(self, rc):
        if rc != _lib.OK:
            last = getattr(self._L, "bigsi_%s_last_error" % self.library)
            raise _lib.BigsiHipError(rc, (last() or b"").decode("utf-8", "replace"))

    def _handle(self):
        if self._h is None:
            raise _lib.BigsiHipError(_lib.ERR_STATE, "the k-mer counter is closed")
        return self._h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:          # (interpreter shutdown)
            pass

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._fn("destroy")(h)

    def reset(self):
        self._check(self._fn("reset")(self._handle()))

    def add_packed(self, blob, offsets):
        """Sequences as one byte blob (bytes or uint8 array) and uint64 offsets[n + 1] into it."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        if n <= 0:
            return
        size = len(blob)
        if int(offsets[-1]) > size or int(offsets[0]) > int(offsets[-1]):
            raise ValueError("offsets reach beyond the %d bytes given" % size)
        if not isinstance(blob, bytes):
            blob = np.ascontiguousarray(blob, dtype=np.uint8)          # (alive until the call below has returned)
        data = blob if isinstance(blob, bytes) else C.cast(C.c_void_p(_lib.ptr(blob) if size else None), C.c_char_p)
        self._check(self._fn("add")(self._handle(), data, _lib.ptr(offsets), n))

    def add(self, seqs):
        """Count the k-mers of an iterable of str or bytes."""
        if isinstance(seqs, (str, bytes)):
            raise TypeError("add() takes an iterable of sequences, not one sequence")
        blob, off = _lib.pack_seqs(seqs)
        self.add_packed(blob, off)

    def add_file(self, path, slice_bytes=SLICE_BYTES):
        """Count the reads of a FASTQ ('@') or FASTA ('>') file, .gz or not, read `slice_bytes` at a time and cut at whole records."""
        opener = gzip.open if str(path).endswith(".gz") else open
        with opener(path, "rb") as f:
            rest = f.read(int(slice_bytes))
            while rest and not rest.strip():          # (empty lines before the first record)
                rest = f.read(int(slice_bytes))
            rest = rest.lstrip()
            if not rest:
                return
            first = rest[:1]
            if first not in (b"@", b">"):
                raise ValueError("%s is neither FASTQ ('@') nor FASTA ('>'): it begins with %r" % (path, first))
            fastq = first == b"@"
            pack = _lib.fastq_pack if fastq else _lib.fasta_pack
            while rest:
                more = f.read(int(slice_bytes))
                cut = record_cut(rest, fastq, not more)
                if cut:
                    packed = pack(rest[:cut])
                    if packed is None:
                        raise ValueError("%s is not plain ASCII" % path)
                    self.add_packed(*packed)
                rest = rest[cut:] + more

    def info(self):
        """{'counted', 'skipped', 'distinct', 'slots'}: positions counted, positions skipped, distinct k-mers, table slots (0 on the host)."""
        out = np.zeros(4, np.uint64)
        self._check(self._fn("info")(self._handle(), _lib.ptr(out)))
        return dict(zip(("counted", "skipped", "distinct", "slots"), (int(x) for x in out)))

    def spectrum(self):
        """uint64[256]: bin c the distinct k-mers seen c times, bin 255 those seen 255 times or more."""
        out = np.zeros(256, np.uint64)
        self._check(self._fn("spectrum")(self._handle(), _lib.ptr(out)))
        return out

    def fetch(self):
        """(uint64 keys, uint32 counts) in ascending key order."""
        n = C.c_uint64(0)
        rc = self._fn("fetch")(self._handle(), None, None, 0, C.byref(n))
        if rc != _lib.ERR_CAPACITY:
            self._check(rc)
        keys, counts = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self._fn("fetch")(self._handle(), _lib.ptr(keys), _lib.ptr(counts), n.value, C.byref(n)))
        return keys, counts

    def bloom_bytes(self, m, h, min_count=1):
        min_count = check_min_count(min_count)
        if int(m) < 1 or int(h) < 1:
            raise ValueError("m and h must be > 0")
        out = np.zeros((int(m) + 7) // 8, np.uint8)
        self._check(self._fn("bloom")(self._handle(), int(m), int(h), min_count, _lib.ptr(out)))
        return out.tobytes()

    def bloom(self, m, h, min_count=1):
        """The m-bit filter (h hashes) of the k-mers seen at least min_count times: BIGSI.bloom of that list, bit for bit."""
        return BitRow.frombytes(self.bloom_bytes(m, h, min_count), int(m))


def spectrum_text(spectrum):
    """The 256 bins as count<TAB>distinct lines."""
    return "".join("%d\t%d\n" % (c, int(n)) for c, n in enumerate(spectrum))


def bloom_from_reads(config, paths_or_seqs, min_count=1, library="hip", spectrum_out=None):
    """The filter of config's (k, m, h) over files and sequences.  An entry is a FILE when it is an os.PathLike, or a str that names an
    existing path; every other str and every bytes entry is a SEQUENCE.  A str sequence that happens to be the name of a file in the
    working directory (a file called "A") would therefore be read as that file: pass sequences as bytes, or files as pathlib.Path,
    where the two are mixed and that could happen."""
    min_count = check_min_count(min_count)
    k = check_k(config["k"])
    device = (config.get("storage-config") or {}).get("device", 0)
    with KmerCounter(k, device=device, library=library) as c:
        seqs = []
        for item in paths_or_seqs:
            if isinstance(item, os.PathLike) or (isinstance(item, str) and os.path.exists(item)):
                c.add_file(os.fspath(item))
            else:
                seqs.append(item)
        if seqs:
            c.add(seqs)
        if spectrum_out is not None:
            spectrum_out.append(c.spectrum())
        return c.bloom(int(config["m"]), int(config["h"]), min_count)
