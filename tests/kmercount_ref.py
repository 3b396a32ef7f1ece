"""The k-mer counter restated (include/bigsi_cpu_kmercount.h, SEMANTICS): a plain Python Counter over canonical k-mers, the spectrum
and the kept list made from it -- plus the planted cases of tests/test_kmercount_host.py (the library's counter, and the conditions
under which no comparison passes vacuously).  No library call: what is here is the definition the library is held against."""
import random
from collections import Counter

MAX_K = 32
LONG = 1024          # a read length well beyond every code-word edge
EMPTY = (1 << 64) - 1

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_DIGITS = bytes.maketrans(b"ACGT", b"0123")
_VALID = frozenset(b"ACGT")


# --------------------------------------------------------------------------------------------- the definition
def canonical(window):
    """The canonical form of an upper-case ACGT window (bytes): the smaller of it and its reverse complement."""
    rc = window.translate(_COMP)[::-1]
    return window if window <= rc else rc


def key_of(kmer):
    """A k-mer's packed key: 2 bits per base, A 0 C 1 G 2 T 3, the first base in the highest used bits."""
    return int(kmer.translate(_DIGITS), 4)


def kmer_of(key, k):
    return "".join("ACGT"[(key >> (2 * (k - 1 - j))) & 3] for j in range(k))


def count(seqs, k):
    """(Counter: canonical key -> occurrences, positions counted, positions skipped) of sequences given as bytes."""
    table, counted, skipped = Counter(), 0, 0
    for s in seqs:
        s = bytes(s).upper()          # (ASCII a-z only: every other byte stays what it is, and is no base)
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if not _VALID.issuperset(w):
                skipped += 1
                continue
            counted += 1
            table[key_of(canonical(w))] += 1
    return table, counted, skipped


def count_periodic(unit, repeats, k):
    """count([unit * repeats], k) for an ACGT unit at least k long, without visiting every window: the window at position p is the one at
    p mod len(unit), so each of the len(unit) windows of unit + unit[:k - 1] occurs as often as its residue lies in [0, positions)."""
    n, positions = len(unit), len(unit) * repeats - k + 1
    assert n >= k and positions > 0 and _VALID.issuperset(unit)
    two, table = unit + unit[:k - 1], Counter()
    for j in range(n):
        times = (positions - j + n - 1) // n
        if times > 0:
            table[key_of(canonical(two[j:j + k]))] += times
    return table, positions, 0


def merge(*results):
    table, counted, skipped = Counter(), 0, 0
    for t, c, s in results:
        table.update(t)
        counted += c
        skipped += s
    return table, counted, skipped


def spectrum(table):
    out = [0] * 256
    for c in table.values():
        out[min(c, 255)] += 1
    return out


def kept(table, k, min_count):
    """The k-mers seen at least min_count times, as upper-case strings in key order: what the filter is the Bloom filter of."""
    return [kmer_of(key, k) for key in sorted(table) if table[key] >= min_count]


def entries(table):
    """[(key, count)] in key order: what a sorted fetch gives."""
    return sorted(table.items())


# --------------------------------------------------------------------------------------------- planted cases
def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


K_EDGES = (1, 2, 15, 16, 17, 31, 32)
LENGTH_KS = (5, 31, 32)


def k_edge_case(k):
    """Reads for one k: random ones over the code-word edges, a homopolymer pair (A^40 and T^40 are one key: 0) and a random tail."""
    rng = random.Random(1000 + k)
    seqs = [rand_seq(rng, n) for n in (k, k + 1, 40, 64, 65, 97, 130)]
    seqs += [b"A" * 40, b"T" * 40, b"A" * 40 + rand_seq(rng, 50)]
    return seqs


def length_edge_case(k):
    rng = random.Random(2000 + k)
    lengths = [k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 95 + k, 96 + k, 97 + k, LONG - 1, LONG, LONG + 1, LONG + k - 1, 2 * LONG + 3, 0]
    return [rand_seq(rng, n) for n in lengths] + [b""]


def invalid_case(k):
    """One 100-base read per way a window can be invalid, the all-N read, NUL and '>' as bytes, and a lower-case twin."""
    rng = random.Random(3000 + k)
    n, seqs = 100, []
    for at in (0, k - 1, k, n - k, n - 1):
        s = bytearray(rand_seq(rng, n))
        s[at] = ord("N")
        seqs.append(bytes(s))
    for gap in (k - 1, k):
        s = bytearray(rand_seq(rng, n))
        s[35] = s[35 + gap] = ord("N")          # (far enough from both ends that every window over either N exists)
        seqs.append(bytes(s))
    seqs.append(b"N" * n)
    for ch in (0, ord(">")):
        s = bytearray(rand_seq(rng, n))
        s[50] = ch
        seqs.append(bytes(s))
    upper = rand_seq(rng, n)
    seqs += [upper, upper.lower(), bytes(c | 0x20 if i % 3 else c for i, c in enumerate(upper))]
    return seqs


COUNT_K = 31
PLANTED_COUNTS = (1, 2, 3, 254, 255, 256)
HOMOPOLYMER_COUNT = 70000
MIN_COUNTS = (1, 2, 3, 255, 256, 70000, 70001)


def count_edge_case():
    """K-mers planted 1, 2, 3, 254, 255 and 256 times (a read of k bases per occurrence, every other one reverse-complemented) and a
    homopolymer read that is 70 000 occurrences of one key."""
    rng = random.Random(4000)
    seqs = []
    for c in PLANTED_COUNTS:
        km = rand_seq(rng, COUNT_K)
        rc = km.translate(_COMP)[::-1]
        seqs += [km if i % 2 == 0 else rc for i in range(c)]
    rng.shuffle(seqs)
    seqs.append(b"C" * (HOMOPOLYMER_COUNT + COUNT_K - 1))
    return seqs


TABLE_K = 31


def table_case():
    """200 reads of 55 bases: 5 000 windows, nearly all distinct."""
    rng = random.Random(5000)
    return [rand_seq(rng, 55) for _ in range(200)]
