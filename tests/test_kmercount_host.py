"""The exact k-mer counter of libbigsi_cpu.so (include/bigsi_cpu_kmercount.h) and the FASTQ packer of libbigsi_hip.so (host only:
include/bigsi_hip_text.h), without a GPU: bigsi_cpu_kmer_counter_* against a plain Python Counter (tests/kmercount_ref.py) at k,
read-length, invalid-byte, count and filter edges and under every cut and order of the input, the conditions the planted cases must
hold so that no comparison passes vacuously, bigsi_hip_fastq_pack on line ends, empty and truncated records, and a stand-alone
sanitized program over the counter."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kmercount_ref as R
from conftest import ROOT
from raw_index import ptr

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_RANGE, ERR_CAPACITY, ERR_STATE = -1, -4, -5, -6


def test_the_empty_sentinel_is_no_key():
    """~0 is no canonical key: T^32 canonicalises to A^32 = 0, and every other 32-mer of all-ones bits does not exist; key 0 is real."""
    assert R.key_of(R.canonical(b"T" * 32)) == 0 == R.key_of(b"A" * 32) and R.key_of(b"T" * 32) == R.EMPTY
    for k in R.K_EDGES:
        assert R.key_of(R.canonical(b"T" * k)) == 0 and all(key < R.EMPTY for key in R.count(R.k_edge_case(k), k)[0])


# --------------------------------------------------------------------------------------------- the cases cannot pass vacuously
def test_count_case_holds_its_planted_counts():
    table, counted, skipped = R.count(R.count_edge_case(), R.COUNT_K)
    counts = sorted(table.values())
    assert counts == sorted(R.PLANTED_COUNTS + (R.HOMOPOLYMER_COUNT,)) and skipped == 0 and counted == sum(counts)
    for c in (2, 255):          # keys at C - 1, C and C + 1: `>=` keeps C, `>` would not
        assert {c - 1, c, c + 1} <= set(counts)
    assert table[R.key_of(b"C" * R.COUNT_K)] == R.HOMOPOLYMER_COUNT          # C^31, not G^31: the canonical one
    spec = R.spectrum(table)
    assert spec[255] == 3 and spec[254] == 1 and spec[0] == 0 and sum(spec) == len(table)
    assert [len(R.kept(table, R.COUNT_K, c)) for c in R.MIN_COUNTS] == [7, 6, 5, 3, 2, 1, 0]
    # a k-mer seen forward in one read and reverse-complemented in another is one key
    seqs = R.count_edge_case()
    assert len(set(seqs[:-1])) == 2 * len(R.PLANTED_COUNTS) - 1          # (the one planted once has no second strand)


def test_invalid_and_edge_cases_hold_what_they_claim():
    for k in (7, 31):
        seqs = R.invalid_case(k)
        table, counted, skipped = R.count(seqs, k)
        assert skipped > 0 and counted > 0
        assert R.count([seqs[7]], k) == ({}, 0, 100 - k + 1)                                     # the all-N read: nothing but skipped windows
        assert R.count([seqs[0]], k)[2] == 1 and R.count([seqs[1]], k)[2] == k and R.count([seqs[2]], k)[2] == k          # N at 0, k - 1, k
        assert R.count([seqs[5]], k)[2] == 2 * k - 1 and R.count([seqs[6]], k)[2] == 2 * k       # two Ns k - 1 and k apart
        assert R.count([seqs[8]], k)[2] == k and R.count([seqs[9]], k)[2] == k                   # NUL and '>'
        assert R.count([seqs[10]], k) == R.count([seqs[11]], k) == R.count([seqs[12]], k) and seqs[11].islower()
    # k = 32: key 0 with count 9 + 9 + 9 from A^40, T^40 and the read that starts with A^40
    table = R.count(R.k_edge_case(32), 32)[0]
    assert table[0] == 27 and R.count([b"A" * 40], 32)[0] == {0: 9} == R.count([b"T" * 40], 32)[0]
    # a palindrome counts once per occurrence
    assert R.count([b"ACGT", b"ACGT"], 4) == ({R.key_of(b"ACGT"): 2}, 2, 0) and R.canonical(b"ACGT") == b"ACGT"
    assert R.count([b"AAAC", b"GTTT"], 4)[0] == {R.key_of(b"AAAC"): 2}
    for k in R.LENGTH_KS:
        lengths = [len(s) for s in R.length_edge_case(k)]
        assert {k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 96 + k, R.LONG - 1, R.LONG, R.LONG + 1, R.LONG + k - 1, 2 * R.LONG + 3, 0} <= set(lengths)


def test_count_periodic_is_count():
    rng = R.random.Random(9)
    unit = R.rand_seq(rng, 40)
    for k, repeats in ((31, 3), (32, 2), (5, 7), (40, 2)):
        assert R.count_periodic(unit, repeats, k) == R.count([unit * repeats], k)


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    P, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name, args in (("create", [C.c_int, u32, u64, C.POINTER(P)]), ("destroy", [P]), ("reset", [P]), ("add", [P, C.c_char_p, P, u64]), ("info", [P, P]),
                       ("spectrum", [P, P]), ("fetch", [P, P, P, u64, C.POINTER(u64)]), ("bloom", [P, u64, u32, u32, P])):
        fn = getattr(L, "bigsi_cpu_kmer_counter_" + name)
        fn.argtypes, fn.restype = args, C.c_int32
    L.bigsi_cpu_bloom.argtypes, L.bigsi_cpu_bloom.restype = [C.c_int, C.c_char_p, u64, u32, u64, u32, u32, P], C.c_int32
    return L


class Twin(object):
    """bigsi_cpu_kmer_counter_* behind the calls the comparisons need."""

    def __init__(self, L, k):
        self.L, self.k, self.h = L, k, C.c_void_p()
        assert L.bigsi_cpu_kmer_counter_create(0, k, 0, C.byref(self.h)) == 0, L.bigsi_cpu_last_error()

    def add(self, seqs):
        blob = b"".join(seqs)
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        return self.L.bigsi_cpu_kmer_counter_add(self.h, blob, ptr(off), len(seqs))

    def info(self):
        out = np.zeros(4, np.uint64)
        assert self.L.bigsi_cpu_kmer_counter_info(self.h, ptr(out)) == 0
        return [int(x) for x in out]

    def spectrum(self):
        out = np.full(256, 7, np.uint64)
        assert self.L.bigsi_cpu_kmer_counter_spectrum(self.h, ptr(out)) == 0
        return [int(x) for x in out]

    def entries(self):
        n = C.c_uint64(0)
        rc = self.L.bigsi_cpu_kmer_counter_fetch(self.h, None, None, 0, C.byref(n))
        assert rc == (ERR_CAPACITY if n.value else 0)
        keys, counts = np.zeros(n.value + 1, np.uint64), np.zeros(n.value + 1, np.uint32)
        assert self.L.bigsi_cpu_kmer_counter_fetch(self.h, ptr(keys), ptr(counts), n.value, C.byref(n)) == 0
        return sorted(zip((int(x) for x in keys[:n.value]), (int(x) for x in counts[:n.value])))

    def bloom(self, m, h, min_count):
        out = np.full((m + 7) // 8 + 1, 0xEE, np.uint8)
        rc = self.L.bigsi_cpu_kmer_counter_bloom(self.h, m, h, min_count, ptr(out))
        assert out[-1] == 0xEE
        return rc, out[:-1].tobytes()

    def close(self):
        assert self.L.bigsi_cpu_kmer_counter_destroy(self.h) == 0


def cpu_bloom(L, kmers, k, m, h):
    out = np.zeros((m + 7) // 8, np.uint8)
    assert L.bigsi_cpu_bloom(0, "".join(kmers).encode(), len(kmers), k, m, h, 0, ptr(out)) == 0
    return out.tobytes()


def check_twin(L, k, adds, want, filters=((1000, 3, 1), (33, 1, 2))):
    t = Twin(L, k)
    for seqs in adds:
        assert t.add(seqs) == 0, L.bigsi_cpu_last_error()
    table, counted, skipped = want
    assert t.info() == [counted, skipped, len(table), 0]
    assert t.entries() == R.entries(table) and t.spectrum() == R.spectrum(table)
    for m, h, c in filters:
        rc, got = t.bloom(m, h, c)
        assert rc == 0 and got == cpu_bloom(L, R.kept(table, k, c), k, m, h), (k, m, h, c)
        if m % 8:
            assert got[-1] & ((1 << (8 - m % 8)) - 1) == 0          # the bits of the last byte past m
    t.close()


@pytest.mark.parametrize("k", R.K_EDGES)
def test_twin_k_edges(cpu, k):
    seqs = R.k_edge_case(k)
    check_twin(cpu, k, [seqs], R.count(seqs, k))


@pytest.mark.parametrize("k", R.LENGTH_KS)
def test_twin_length_edges(cpu, k):
    seqs = R.length_edge_case(k)
    check_twin(cpu, k, [seqs, []], R.count(seqs, k))


@pytest.mark.parametrize("k", (7, 31))
def test_twin_invalid_bytes(cpu, k):
    seqs = R.invalid_case(k)
    check_twin(cpu, k, [seqs], R.count(seqs, k))


def test_twin_count_and_filter_edges(cpu):
    seqs = R.count_edge_case()
    want = R.merge(R.count(seqs[:-1], R.COUNT_K), R.count_periodic(b"C" * R.COUNT_K, (len(seqs[-1]) // R.COUNT_K), R.COUNT_K),
                   R.count([b"C" * (R.COUNT_K - 1 + len(seqs[-1]) % R.COUNT_K)], R.COUNT_K))
    assert want[0][R.key_of(b"C" * R.COUNT_K)] == R.HOMOPOLYMER_COUNT and want[1] == sum(R.PLANTED_COUNTS) + R.HOMOPOLYMER_COUNT
    filters = [(1000, 3, c) for c in R.MIN_COUNTS] + [(m, h, 2) for m in (7, 8, 33, 1000, (1 << 20) + 1) for h in (1, 3, 7)]
    check_twin(cpu, R.COUNT_K, [seqs], want, filters)


def test_twin_table_and_order_cases(cpu):
    reads = R.table_case()
    want = R.count(reads, R.TABLE_K)
    for adds in ([reads], [reads[i::7] for i in range(7)], [[r] for r in reads], [reads[::-1]]):
        check_twin(cpu, R.TABLE_K, adds, want)


def test_twin_refusals(cpu):
    h = C.c_void_p()
    assert cpu.bigsi_cpu_kmer_counter_create(0, 33, 0, C.byref(h)) == ERR_INVALID and b"33" in cpu.bigsi_cpu_last_error() and not h
    assert cpu.bigsi_cpu_kmer_counter_create(0, 0, 0, C.byref(h)) == ERR_INVALID and cpu.bigsi_cpu_kmer_counter_create(0, 5, 0, None) == ERR_INVALID
    t = Twin(cpu, 5)
    off = np.array([0, 9], np.uint64)
    assert cpu.bigsi_cpu_kmer_counter_add(None, b"ACGTACGTA", ptr(off), 1) == ERR_INVALID and cpu.bigsi_cpu_kmer_counter_add(t.h, b"ACGTACGTA", None, 1) == ERR_INVALID
    assert cpu.bigsi_cpu_kmer_counter_add(t.h, None, ptr(off), 1) == ERR_INVALID and cpu.bigsi_cpu_kmer_counter_add(t.h, None, None, 0) == 0
    assert cpu.bigsi_cpu_kmer_counter_add(t.h, b"ACGTACGTA", ptr(np.array([9, 0], np.uint64)), 1) == ERR_INVALID
    # offsets that claim 2^32 + 4 bytes -- 2^32 windows of k = 5, one more than a counter takes in its lifetime: refused from the
    # offsets alone (the nine bytes behind seqs are never read); 2^32 - 1 windows would be taken
    assert cpu.bigsi_cpu_kmer_counter_add(t.h, b"ACGTACGTA", ptr(np.array([0, (1 << 32) + 4], np.uint64)), 1) == ERR_RANGE and b"2^32" in cpu.bigsi_cpu_last_error()
    assert t.info() == [0, 0, 0, 0]
    assert t.add([b"ACGTACGTA"]) == 0 and t.bloom(100, 3, 0)[0] == ERR_INVALID and t.bloom(100, 0, 1)[0] == ERR_INVALID
    assert cpu.bigsi_cpu_kmer_counter_bloom(t.h, 0, 3, 1, ptr(np.zeros(1, np.uint8))) == ERR_INVALID
    assert cpu.bigsi_cpu_kmer_counter_info(t.h, None) == ERR_INVALID and cpu.bigsi_cpu_kmer_counter_spectrum(None, None) == ERR_INVALID
    keys, counts, n = np.full(8, 0xAB, np.uint64), np.full(8, 0xAB, np.uint32), C.c_uint64(0)
    assert cpu.bigsi_cpu_kmer_counter_fetch(t.h, ptr(keys), ptr(counts), 1, C.byref(n)) == ERR_CAPACITY and n.value == 2 == len(R.count([b"ACGTACGTA"], 5)[0])
    assert (keys == 0xAB).all() and (counts == 0xAB).all()          # a sizing call writes nothing
    t.close()


# --------------------------------------------------------------------------------------------- the FASTQ packer
def fastq_pack(text, max_records=None):
    from bigsi_amd import _lib
    n = C.c_uint64(0)
    rc = _lib.lib().bigsi_hip_fastq_pack(text, len(text), None, None, 0, C.byref(n))
    if rc:
        return rc, (_lib.lib().bigsi_hip_last_error() or b"").decode()
    blob, off = np.full(len(text) + 1, 0x7E, np.uint8), np.zeros(n.value + 1, np.uint64)
    rc = _lib.lib().bigsi_hip_fastq_pack(text, len(text), ptr(blob), ptr(off), n.value if max_records is None else max_records, C.byref(n))
    if rc:
        return rc, (_lib.lib().bigsi_hip_last_error() or b"").decode()
    assert blob[int(off[-1])] == 0x7E
    return 0, [bytes(blob[int(a):int(b)]) for a, b in zip(off, off[1:])]


def test_fastq_pack():
    recs = [(b"r1", b"ACGTN", b"IIII#"), (b"r2 extra words", b"", b""), (b"r3", b"acgtACGT", b"@+@+@+@+"), (b"r4", b"T", b"@")]
    for eol in (b"\n", b"\r\n", b"\r"):
        text = b"".join(b"@" + n + eol + s + eol + b"+" + eol + q + eol for n, s, q in recs)
        assert fastq_pack(text) == (0, [s for _, s, _ in recs]), eol
        assert fastq_pack(text[:-len(eol)]) == (0, [s for _, s, _ in recs])          # no line end behind the last line
        assert fastq_pack(text + eol + eol) == (0, [s for _, s, _ in recs])          # empty lines behind the last record
    assert fastq_pack(b"") == (0, []) and fastq_pack(b"\n\n") == (0, [])
    assert fastq_pack(b"@r\n\n+\n") == (0, [b""]) and fastq_pack(b"@r\n\n+") == (0, [b""])          # an empty sequence, an empty quality line cut off
    assert fastq_pack(b"@a\nAC\n+a\nII\n@b\nGT\n+\n@I\n") == (0, [b"AC", b"GT"])          # '@' as the first quality character; '+name' lines
    for text, record, why in ((b"@a\nAC\n+\nII\n@b\nGT\n+\n", 2, "ends inside"), (b"@a\nAC\n+\nII\n@b\nGT\n", 2, "ends inside"), (b"@a\nAC\n+\nII\n@b", 2, "ends inside"),
                              (b"@a\nAC\n+\nI\n", 1, "quality"), (b">a\nACGT\n", 1, "'@'"), (b"@a\nAC\nGT\n+\nIIII\n", 1, "'+'"),
                              (b"@a\nAC\n+\nII\n@b\nG\xc3\x9cT\n+\nIII\n", 2, "0x80"), (b"@a\nAC\n+\nII\nACGT\n", 2, "'@'")):
        rc, msg = fastq_pack(text)
        assert rc == ERR_INVALID and "record %d" % record in msg and why in msg, (text, msg)
    text = b"@a\nAC\n+\nII\n@b\nGT\n+\nII\n"
    assert fastq_pack(text, max_records=1)[0] == ERR_CAPACITY
    from bigsi_amd import _lib
    assert _lib.lib().bigsi_hip_fastq_pack(None, 5, None, None, 0, C.byref(C.c_uint64())) == ERR_INVALID and _lib.lib().bigsi_hip_fastq_pack(text, len(text), None, None, 0, None) == ERR_INVALID
    blob, off = _lib.fastq_pack(text)
    assert bytes(blob) == b"ACGT" and off.tolist() == [0, 2, 4]
    with pytest.raises(_lib.BigsiHipError, match="record 1"):
        _lib.fastq_pack(b"nothing of the kind")


def test_abi_lists_the_new_entry_points():
    from bigsi_amd import _lib
    text_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_text.h")).read(), flags=re.S)
    public = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip.h")).read(), flags=re.S)
    assert "bigsi_hip_fastq_pack(" in text_h and "bigsi_hip_fastq_pack" not in public
    assert _lib.SIGNATURES["bigsi_hip_fastq_pack"] == _lib.SIGNATURES["bigsi_hip_fasta_pack"]
    twin = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_cpu_kmercount.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bigsi_cpu_kmer_counter_\w+)\s*\(", twin))) == ["bigsi_cpu_kmer_counter_" + n for n in
                                                                                 ("add", "bloom", "create", "destroy", "fetch", "info", "reset", "spectrum")]
    assert "#define BIGSI_KMERCOUNT_MAX_K 32u" in twin and R.MAX_K == 32


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_the_counter(tmp_path):
    """tests/c_host/kmercount_sanitize_main.cpp -- a program with its own main that drives bigsi_cpu_kmer_counter_* over odd shapes -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own."""
    exe = str(tmp_path / "kmercount_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "kmercount_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "kmercount: ok", (r.stdout[-1000:], r.stderr[-3000:])
