"""The exact k-mer counter on the device (include/bigsi_hip_kmercount.h), straight on the C ABI: k_count_kmers and k_kmer_table_rehash /
spectrum / bloom / fetch against the Python restatement (tests/kmercount_ref.py) and against the host twin (libbigsi_cpu.so) -- every
k of K_EDGES, read lengths and invalid bytes around the code-word edges, N bytes around the edges of the counting kernel's tile,
planted counts up to a 70 000-fold homopolymer, every filter byte for byte bigsi_hip_bloom of the kept k-mers, a table that grows
several times under a 4096-byte staging chunk in 1, 7 and 200 calls and in reversed order, reset, the refusals, and the KmerCounter
class over a gzipped FASTQ file.  tests/test_kmercount_host.py asserts, on the CPU, that none of the planted cases is vacuous.

Every add whose offsets reach beyond its buffer goes through claim_beyond(), which works out from the restatement's arithmetic that the
call must be refused (more than 2^32 - 1 - taken positions, or decreasing offsets) and raises instead of calling when it would not be:
an accepted call reads every byte it names."""
import ctypes as C
import gzip

import numpy as np
import pytest

import kmercount_ref as R
from raw_index import ptr
from test_kmercount_host import Twin, cpu  # noqa: F401  (cpu: the fixture that loads libbigsi_cpu.so)

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_RANGE, ERR_CAPACITY, ERR_STATE = -1, -4, -5, -6
LIFETIME = (1 << 32) - 1
TILE = 4096          # kKmerTile (tests/test_kmercount_plan_host.py pins it)


@pytest.fixture(scope="module")
def L():
    from bigsi_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible"
    return _lib.lib()


def last_error(L):
    return (L.bigsi_hip_last_error() or b"").decode()


class Dev(object):
    """bigsi_hip_kmer_counter_* behind the calls the comparisons need."""

    def __init__(self, L, k, expected=0, limits=None):
        self.L, self.k, self.h = L, k, C.c_void_p()
        assert L.bigsi_hip_kmer_counter_create(0, k, expected, C.byref(self.h)) == 0, last_error(L)
        if limits:
            assert L.bigsi_hip_kmer_counter_set_limits(self.h, *limits) == 0, last_error(L)

    def add(self, seqs):
        """A truthful call: the offsets name exactly the bytes of the blob."""
        blob = b"".join(seqs)
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        assert int(off[-1]) == len(blob)
        rc = self.L.bigsi_hip_kmer_counter_add(self.h, blob, ptr(off), len(seqs))
        assert rc == 0, last_error(self.L)

    def info(self):
        out = np.zeros(4, np.uint64)
        assert self.L.bigsi_hip_kmer_counter_info(self.h, ptr(out)) == 0
        return [int(x) for x in out]

    def spectrum(self):
        out = np.full(256, 7, np.uint64)
        assert self.L.bigsi_hip_kmer_counter_spectrum(self.h, ptr(out)) == 0, last_error(self.L)
        return [int(x) for x in out]

    def entries(self):
        """As fetched: the order is the library's."""
        n = C.c_uint64(0)
        rc = self.L.bigsi_hip_kmer_counter_fetch(self.h, None, None, 0, C.byref(n))
        assert rc == (ERR_CAPACITY if n.value else 0)
        keys, counts = np.full(n.value + 1, 0xAB, np.uint64), np.full(n.value + 1, 0xAB, np.uint32)
        assert self.L.bigsi_hip_kmer_counter_fetch(self.h, ptr(keys), ptr(counts), n.value, C.byref(n)) == 0, last_error(self.L)
        assert keys[-1] == 0xAB and counts[-1] == 0xAB
        return list(zip((int(x) for x in keys[:-1]), (int(x) for x in counts[:-1])))

    def bloom(self, m, h, min_count):
        out = np.full((m + 7) // 8 + 1, 0xEE, np.uint8)
        rc = self.L.bigsi_hip_kmer_counter_bloom(self.h, m, h, min_count, ptr(out))
        assert out[-1] == 0xEE
        return rc, out[:-1].tobytes()

    def reset(self):
        assert self.L.bigsi_hip_kmer_counter_reset(self.h) == 0, last_error(self.L)

    def close(self):
        assert self.L.bigsi_hip_kmer_counter_destroy(self.h) == 0


def hip_bloom(L, kmers, k, m, h):
    """bigsi_hip_bloom of a k-mer list: what the counter's filter is held against."""
    out = np.zeros((m + 7) // 8, np.uint8)
    assert L.bigsi_hip_bloom(0, "".join(kmers).encode(), len(kmers), k, m, h, 0, ptr(out)) == 0, last_error(L)
    return out.tobytes()


def check_dev(L, d, want, filters=((1000, 3, 1), (33, 1, 2)), slots_at_least=64):
    table, counted, skipped = want
    info = d.info()
    assert info[:3] == [counted, skipped, len(table)]
    assert info[3] >= slots_at_least and info[3] & (info[3] - 1) == 0 and 2 * len(table) <= info[3]
    got = d.entries()
    assert got == R.entries(table)          # ascending key order, as fetched
    assert all(key != R.EMPTY for key, _ in got)
    assert d.spectrum() == R.spectrum(table)
    for m, h, c in filters:
        rc, bits = d.bloom(m, h, c)
        assert rc == 0 and bits == hip_bloom(L, R.kept(table, d.k, c), d.k, m, h), (d.k, m, h, c)
        if m % 8:
            assert bits[-1] & ((1 << (8 - m % 8)) - 1) == 0          # the bits of the last byte past m


def check_against_twin(L, cpu, k, adds, want, filters=((1000, 3, 1), (33, 1, 2))):
    d, t = Dev(L, k), Twin(cpu, k)
    for seqs in adds:
        d.add(seqs)
        assert t.add(seqs) == 0
    check_dev(L, d, want, filters)
    assert d.info()[:3] == t.info()[:3] and d.entries() == t.entries() and d.spectrum() == t.spectrum()
    for m, h, c in filters:
        assert d.bloom(m, h, c) == t.bloom(m, h, c)
    d.close()
    t.close()


# --------------------------------------------------------------------------------------------- k, length and invalid-byte edges
@pytest.mark.parametrize("k", R.K_EDGES)
def test_k_edges(L, cpu, k):
    seqs = R.k_edge_case(k)
    want = R.count(seqs, k)
    assert want[0][0] >= 3 * (40 - k + 1) and R.EMPTY not in want[0]          # A^40 and T^40 (and the read that starts with A^40) are one key 0
    check_against_twin(L, cpu, k, [seqs], want)


@pytest.mark.parametrize("k", R.LENGTH_KS)
def test_length_edges(L, cpu, k):
    seqs = R.length_edge_case(k)
    check_against_twin(L, cpu, k, [seqs, []], R.count(seqs, k))


@pytest.mark.parametrize("k", R.LENGTH_KS)
def test_invalid_bytes(L, cpu, k):
    seqs = R.invalid_case(k)
    want = R.count(seqs, k)
    assert want[2] > 0
    check_against_twin(L, cpu, k, [seqs], want)


def tile_edge_reads(k):
    """Reads that lie at the start of their call's staged stream, so that read position p is window start p of the counting kernel: N at
    the window starts TILE - 1, TILE and TILE + 1, and one N exactly k - 1 before a tile edge (the first valid window behind it starts
    one base later and reads across the edge)."""
    rng = R.random.Random(6000 + k)
    around = bytearray(R.rand_seq(rng, 5000))
    for p in (TILE - 1, TILE, TILE + 1):
        around[p] = ord("N")
    before = bytearray(R.rand_seq(rng, 5000))
    before[TILE - (k - 1)] = ord("N")
    both = bytearray(R.rand_seq(rng, 2 * TILE + 900))
    for p in (TILE - 1, TILE, TILE + 1, 2 * TILE - (k - 1)):
        both[p] = ord("N")
    clean = R.rand_seq(rng, 2 * TILE + k - 1)          # its last window starts at 2 * TILE: a tile of one start
    return [bytes(around), bytes(before), bytes(both), clean]


@pytest.mark.parametrize("k", R.LENGTH_KS)
def test_tile_edges(L, cpu, k):
    reads = tile_edge_reads(k)
    assert R.count(reads[:1], k)[2] == k + 2 and R.count(reads[1:2], k)[2] == k and R.count(reads[2:3], k)[2] == 2 * k + 2
    for r in reads:          # each alone: position p of the read is window start p of the kernel
        check_against_twin(L, cpu, k, [[r]], R.count([r], k))
    check_against_twin(L, cpu, k, [reads, reads[::-1]], R.merge(R.count(reads, k), R.count(reads, k)))


# --------------------------------------------------------------------------------------------- counts, spectrum, fetch, filters
def count_edge_want():
    seqs = R.count_edge_case()
    want = R.merge(R.count(seqs[:-1], R.COUNT_K), R.count_periodic(b"C" * R.COUNT_K, (len(seqs[-1]) // R.COUNT_K), R.COUNT_K),
                   R.count([b"C" * (R.COUNT_K - 1 + len(seqs[-1]) % R.COUNT_K)], R.COUNT_K))
    assert want[0][R.key_of(b"C" * R.COUNT_K)] == R.HOMOPOLYMER_COUNT and want[1] == sum(R.PLANTED_COUNTS) + R.HOMOPOLYMER_COUNT
    return seqs, want


def test_count_and_filter_edges(L, cpu):
    seqs, want = count_edge_want()
    filters = [(1000, 3, c) for c in R.MIN_COUNTS] + [(m, h, c) for c in R.MIN_COUNTS for m in (7, 8, 33, 1000, (1 << 20) + 1) for h in (1, 3, 7)]
    d = Dev(L, R.COUNT_K)
    d.add(seqs)
    check_dev(L, d, want, filters)
    spec = d.spectrum()
    assert spec[255] == 3 and spec[254] == 1 and spec[0] == 0 and sum(spec) == 7          # 255, 256 and 70 000 share the last bin
    assert sorted(c for _, c in d.entries()) == sorted(R.PLANTED_COUNTS + (R.HOMOPOLYMER_COUNT,))
    assert d.bloom(1000, 3, R.HOMOPOLYMER_COUNT + 1) == (0, bytes(125))                     # nothing is kept: an all-zero filter
    t = Twin(cpu, R.COUNT_K)
    assert t.add(seqs) == 0 and t.entries() == d.entries() and t.spectrum() == spec
    t.close()
    d.close()


# --------------------------------------------------------------------------------------------- table growth, chunk cuts, order
def test_table_growth_cuts_and_order(L):
    long_read = R.rand_seq(R.random.Random(77), 9001)          # longer than two staging chunks
    reads = R.table_case() + [long_read]
    want = R.count(reads, R.TABLE_K)
    assert len(want[0]) > 8000
    for adds in ([reads], [reads[i::7] for i in range(7)], [[r] for r in reads[:200]] + [[long_read]], [reads[::-1]]):
        d = Dev(L, R.TABLE_K, limits=(4096, 64))
        assert d.info() == [0, 0, 0, 64]
        grown = [64]
        for seqs in adds:
            d.add(seqs)
            grown.append(d.info()[3])
        assert grown == sorted(grown) and grown[-1] >= 1 << 15, grown                                   # info()[3] grew
        assert len(adds) < 7 or len(set(grown)) >= 4, grown                                             # ... call after call, several times
        check_dev(L, d, want)
        d.close()
    # the same through the library's own chunk and table, and with a sizing hint
    for expected in (0, 9000):
        d = Dev(L, R.TABLE_K, expected=expected)
        d.add(reads)
        check_dev(L, d, want, slots_at_least=1 << 16)
        d.close()


def test_reset_and_recount(L):
    seqs = R.k_edge_case(17)
    d = Dev(L, 17, limits=(4096, 64))
    d.add(R.table_case())
    assert d.info()[3] > 64
    d.reset()
    assert d.info() == [0, 0, 0, 64] and d.entries() == [] and d.spectrum() == [0] * 256 and d.bloom(100, 3, 1) == (0, bytes(13))
    d.add(seqs)
    check_dev(L, d, R.count(seqs, 17))
    d.reset()
    d.add(seqs + seqs)
    check_dev(L, d, R.merge(R.count(seqs, 17), R.count(seqs, 17)))
    assert L.bigsi_hip_kmer_counter_set_limits(d.h, 0, 0) == ERR_STATE          # it holds k-mers
    d.close()


# --------------------------------------------------------------------------------------------- refusals
def claim_beyond(d, blob, offsets, taken):
    """An add whose offsets reach beyond `blob`.  From the restatement's arithmetic -- positions are sum(len - k + 1), a counter takes
    2^32 - 1 in its lifetime, decreasing offsets are refused first -- the call must be refused before a byte is read; if it would be
    accepted, this raises instead of calling."""
    k = d.k
    decreasing = any(b < a for a, b in zip(offsets, offsets[1:]))
    positions = sum(max(b - a - k + 1, 0) for a, b in zip(offsets, offsets[1:]))
    if not decreasing and not positions > LIFETIME - taken:
        raise AssertionError("offsets %r claim %d positions behind %d taken: the call would be accepted and read bytes it does not own" % (offsets, positions, taken))
    assert d.info()[0] + d.info()[1] == taken
    return d.L.bigsi_hip_kmer_counter_add(d.h, blob, ptr(np.asarray(offsets, np.uint64)), len(offsets) - 1)


def test_claim_beyond_refuses_to_make_an_accepted_call():
    class Never(object):
        k = 5
    with pytest.raises(AssertionError, match="would be accepted"):
        claim_beyond(Never(), b"ACGTACGTA", [0, (1 << 32) + 3], 0)          # 2^32 - 1 windows: exactly what a counter takes
    with pytest.raises(AssertionError, match="would be accepted"):
        claim_beyond(Never(), b"ACGTACGTA", [0, 10], 0)


def test_refusals(L):
    h = C.c_void_p()
    assert L.bigsi_hip_kmer_counter_create(0, 33, 0, C.byref(h)) == ERR_INVALID and "33" in last_error(L) and not h
    assert L.bigsi_hip_kmer_counter_create(0, 0, 0, C.byref(h)) == ERR_INVALID and L.bigsi_hip_kmer_counter_create(0, 5, 0, None) == ERR_INVALID
    d = Dev(L, 5)
    nine = b"ACGTACGTA"
    off = np.array([0, 9], np.uint64)
    assert L.bigsi_hip_kmer_counter_add(None, nine, ptr(off), 1) == ERR_INVALID and L.bigsi_hip_kmer_counter_add(d.h, nine, None, 1) == ERR_INVALID
    assert L.bigsi_hip_kmer_counter_add(d.h, None, ptr(off), 1) == ERR_INVALID and L.bigsi_hip_kmer_counter_add(d.h, None, None, 0) == 0
    assert claim_beyond(d, nine, [9, 0], 0) == ERR_INVALID
    # 2^32 + 4 bytes at k = 5 are 2^32 windows, one more than a counter takes: refused from the offsets alone
    assert claim_beyond(d, nine, [0, (1 << 32) + 4], 0) == ERR_RANGE and "2^32" in last_error(L)
    assert d.info()[:3] == [0, 0, 0]
    d.add([nine])                                                            # a truthful add: 5 positions
    assert d.info()[:3] == [5, 0, 2]
    assert claim_beyond(d, nine, [0, LIFETIME - 5 + 5], 5) == ERR_RANGE      # 2^32 - 5 windows behind 5 taken: one over
    assert d.info()[:3] == [5, 0, 2] and d.entries() == R.entries(R.count([nine], 5)[0])
    assert d.bloom(100, 3, 0)[0] == ERR_INVALID and d.bloom(100, 0, 1)[0] == ERR_INVALID
    assert L.bigsi_hip_kmer_counter_bloom(d.h, 0, 3, 1, ptr(np.zeros(1, np.uint8))) == ERR_INVALID
    assert L.bigsi_hip_kmer_counter_info(d.h, None) == ERR_INVALID and L.bigsi_hip_kmer_counter_spectrum(None, None) == ERR_INVALID
    keys, counts, n = np.full(8, 0xAB, np.uint64), np.full(8, 0xAB, np.uint32), C.c_uint64(0)
    assert L.bigsi_hip_kmer_counter_fetch(d.h, ptr(keys), ptr(counts), 1, C.byref(n)) == ERR_CAPACITY and n.value == 2
    assert (keys == 0xAB).all() and (counts == 0xAB).all()          # a sizing call writes nothing
    for chunk, slots in ((63, 0), (0, 63), (0, 96), (0, 32)):
        assert L.bigsi_hip_kmer_counter_set_limits(d.h, chunk, slots) == ERR_STATE          # it holds k-mers: state before values
    d.reset()
    for chunk, slots in ((63, 0), (0, 96), (0, 32), (1, 64)):
        assert L.bigsi_hip_kmer_counter_set_limits(d.h, chunk, slots) == ERR_INVALID
    assert L.bigsi_hip_kmer_counter_set_limits(d.h, 64, 128) == 0 and d.info() == [0, 0, 0, 128]
    assert L.bigsi_hip_kmer_counter_set_limits(None, 0, 0) == ERR_INVALID
    d.close()
    assert L.bigsi_hip_kmer_counter_destroy(None) == 0


# --------------------------------------------------------------------------------------------- the class
def test_class_over_both_libraries(L, tmp_path):
    from bigsi_amd.graph.bigsi import BIGSI
    from bigsi_amd.kmercount import KmerCounter
    k = 21
    rng = R.random.Random(8)
    reads = [R.rand_seq(rng, n) for n in (150, 150, 20, 21, 400)] * 3 + [b"ACGTN" * 30, b"acgtacgtacgtacgtacgtacgtacgt", R.rand_seq(rng, 60), R.rand_seq(rng, 77) * 2]
    want = R.count(reads, k)
    path = str(tmp_path / "reads.fastq.gz")
    with gzip.open(path, "wb") as f:
        f.write(b"".join(b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(reads)))
    got = {}
    for library in ("hip", "cpu"):
        with KmerCounter(k, library=library) as c:
            c.add_file(path, slice_bytes=700)
            info = c.info()
            assert [info["counted"], info["skipped"], info["distinct"]] == [want[1], want[2], len(want[0])] and (info["slots"] > 0) == (library == "hip")
            keys, counts = c.fetch()
            assert list(zip(keys.tolist(), counts.tolist())) == R.entries(want[0]) and c.spectrum().tolist() == R.spectrum(want[0])
            got[library] = [c.bloom(5003, 3, mc).tobytes() for mc in (1, 2, 3, 4)]
    assert got["hip"] == got["cpu"] and len(set(got["hip"])) >= 3
    config = {"k": k, "m": 5003, "h": 3}
    for mc in (1, 3):
        row = BIGSI.bloom_from_reads(config, [path], min_count=mc)
        assert row.tobytes() == BIGSI.bloom(config, R.kept(want[0], k, mc)).tobytes() == got["hip"][mc - 1]
    assert BIGSI.bloom_from_reads(config, [r.decode() for r in reads], 1).tobytes() == got["hip"][0]
