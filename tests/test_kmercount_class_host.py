"""bigsi_amd/kmercount.py without a GPU: KmerCounter(library="cpu") -- the class the device counter is driven through, over the host
twin -- against the Python restatement (tests/kmercount_ref.py): refusals, add() of str and bytes, add_file() on FASTQ and FASTA text
with LF and CR LF line ends and through gzip, at slice sizes of one record, three records and the whole file, the spectrum file, the
binding of the device header, and what the `bloom` command decides from its arguments before any device work."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import kmercount_ref as R
from conftest import ROOT

from bigsi_amd import _lib, kmercount
from bigsi_amd.kmercount import KmerCounter

K = 7
READS = [b"ACGTACGTTGCA", b"ACGTNACGTTGCAAC", b"", b"acgtacgttgcaGGA", b"TTTTTTTTTT", b"GATTACA", b"GATTAC", b"CCCCCCCCCCCCCCCCCCCCC", b"ACGTTGCATGCATGCAAT",
         b"TGCAACGTACGT", b"GGGGGGGGGG"]


def fastq_text(reads, eol=b"\n"):
    return b"".join(b"@r%d some words" % i + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for i, s in enumerate(reads))


def fasta_text(reads, eol=b"\n", width=5):
    out = []
    for i, s in enumerate(reads):
        out.append(b">s%d" % i + eol)
        out.extend(s[j:j + width] + eol for j in range(0, len(s), width))
    return b"".join(out)


def cpu_bloom(kmers, k, m, h):
    L = kmercount.load_library("cpu")
    L.bigsi_cpu_bloom.argtypes, L.bigsi_cpu_bloom.restype = [C.c_int, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p], C.c_int32
    out = np.zeros((m + 7) // 8, np.uint8)
    assert L.bigsi_cpu_bloom(0, "".join(kmers).encode(), len(kmers), k, m, h, 0, _lib.ptr(out)) == 0
    return out.tobytes()


def check_counter(c, k, want):
    table, counted, skipped = want
    assert c.info() == {"counted": counted, "skipped": skipped, "distinct": len(table), "slots": 0}
    keys, counts = c.fetch()
    assert keys.dtype == np.uint64 and counts.dtype == np.uint32 and list(zip(keys.tolist(), counts.tolist())) == R.entries(table)
    assert c.spectrum().tolist() == R.spectrum(table)
    for m, h, mc in ((1000, 3, 1), (33, 1, 2), (64, 2, 3)):
        row = c.bloom(m, h, mc)
        assert row.tobytes() == c.bloom_bytes(m, h, mc) == cpu_bloom(R.kept(table, k, mc), k, m, h) and len(row) == m


def test_the_reads_hold_what_the_checks_need():
    table, counted, skipped = R.count(READS, K)
    assert skipped > 0 and max(table.values()) >= 3 and min(table.values()) == 1 and {1, 2} <= set(table.values())
    assert len(R.kept(table, K, 1)) > len(R.kept(table, K, 2)) > len(R.kept(table, K, 3)) > 0


def test_add_str_bytes_and_cuts():
    want = R.count(READS, K)
    with KmerCounter(K, library="cpu") as c:
        c.add(READS)
        check_counter(c, K, want)
        c.reset()
        assert c.info()["counted"] == 0 and c.fetch()[0].size == 0
        for i, s in enumerate(READS):          # one call each, str and bytes alternating
            c.add([s.decode() if i % 2 else s])
        c.add([])
        c.add(iter(()))
        check_counter(c, K, want)
    with KmerCounter(K, expected_distinct=10, device=0, library="cpu") as c:
        c.add(s.decode() for s in reversed(READS))
        check_counter(c, K, want)
        blob = np.frombuffer(b"xx" + b"".join(READS), np.uint8)
        c.reset()
        c.add_packed(blob, np.array([2] + [2 + x for x in np.cumsum([len(s) for s in READS])], np.uint64))          # offsets[0] > 0, a numpy blob
        check_counter(c, K, want)


def test_refusals():
    for bad, err in ((0, ValueError), (33, ValueError), (-1, ValueError), (True, TypeError), (31.0, TypeError), ("31", TypeError)):
        with pytest.raises(err):
            KmerCounter(bad, library="cpu")
    with pytest.raises(ValueError, match="'hip' or 'cpu'"):
        KmerCounter(31, library="auto")
    c = KmerCounter(K, library="cpu")
    for bad in ("ACGTACGTAC", b"ACGTACGTAC"):
        with pytest.raises(TypeError):
            c.add(bad)
    with pytest.raises(ValueError, match="ASCII"):
        c.add(["ACGTÜ"])
    with pytest.raises(ValueError, match="beyond"):          # the class never hands the library offsets beyond the buffer it passes
        c.add_packed(b"ACGTACGTA", np.array([0, (1 << 32) + 4], np.uint64))
    with pytest.raises(ValueError, match="beyond"):
        c.add_packed(b"ACGTACGTA", np.array([0, 10], np.uint64))
    with pytest.raises(_lib.BigsiHipError, match="non-decreasing") as e:
        c.add_packed(b"ACGTACGTA", np.array([0, 9, 4, 9], np.uint64))
    assert e.value.code == _lib.ERR_INVALID and c.info()["counted"] == 0
    for m, h, mc, err in ((0, 3, 1, ValueError), (100, 0, 1, ValueError), (100, 3, 0, ValueError), (100, 3, -2, ValueError), (100, 3, 1 << 32, ValueError),
                          (100, 3, 1.0, TypeError), (100, 3, True, TypeError)):
        with pytest.raises(err):
            c.bloom(m, h, mc)
    c.close()
    c.close()
    for call in (c.info, c.spectrum, c.fetch, c.reset, lambda: c.add([b"ACGTACGTA"]), lambda: c.bloom(10, 1)):
        with pytest.raises(_lib.BigsiHipError, match="closed"):
            call()


@pytest.mark.parametrize("eol", (b"\n", b"\r\n", b"\r"))
@pytest.mark.parametrize("fastq", (True, False))
def test_add_file(tmp_path, eol, fastq):
    text = fastq_text(READS, eol) if fastq else fasta_text(READS, eol)
    want = R.count(READS, K)
    record = len(text) // len(READS)
    plain, gz = str(tmp_path / "reads.txt"), str(tmp_path / "reads.txt.gz")
    open(plain, "wb").write(text)
    with gzip.open(gz, "wb") as f:
        f.write(text)
    for path in (plain, gz):
        for slice_bytes in (1, record, 3 * record, 7, len(text), len(text) + 1, 1 << 20):          # one record or less, three, the whole file
            with KmerCounter(K, library="cpu") as c:
                c.add_file(path, slice_bytes=slice_bytes)
                check_counter(c, K, want)
    # empty lines before the first record and behind the last one; a file without the last line end
    for body in (eol + eol + text + eol, text[:-len(eol)]):
        open(plain, "wb").write(body)
        with KmerCounter(K, library="cpu") as c:
            c.add_file(plain, slice_bytes=11)
            check_counter(c, K, want)


def test_add_file_refusals_and_empty(tmp_path):
    path = str(tmp_path / "x")
    with KmerCounter(K, library="cpu") as c:
        for body in (b"", b"\n\n"):
            open(path, "wb").write(body)
            c.add_file(path)
        assert c.info()["counted"] == 0
        open(path, "wb").write(b"ACGTACGT\nACGTTTTT\n")
        with pytest.raises(ValueError, match="neither FASTQ"):
            c.add_file(path)
        open(path, "wb").write(b"@r\nACGTACGTAC\n+\nIII\n")          # quality of another length
        with pytest.raises(_lib.BigsiHipError, match="record 1"):
            c.add_file(path)
        with pytest.raises(OSError):
            c.add_file(str(tmp_path / "missing.fastq"))


def test_record_cut():
    cut = kmercount.record_cut
    fq = fastq_text([b"ACGT", b"GG"])
    first = len(fastq_text([b"ACGT"]))
    assert cut(fq, True, True) == len(fq) and cut(fq, True, False) == len(fq) and cut(fq[:-1], True, False) == first and cut(fq[:first - 1], True, False) == 0
    fa = fasta_text([b"ACGTACGT", b"GG"])
    assert cut(fa, False, True) == len(fa) and fa[cut(fa, False, False):] == b">s1\nGG\n" and cut(b">s0\nACGT\nAC", False, False) == 0
    cr = fastq_text([b"ACGT", b"GG"], b"\r")                 # CR-only line ends, which the packer takes: cut at CR where there is no LF
    assert cut(cr, True, False) == len(cr) and cut(cr[:-1], True, False) == first and cut(cr[:3], True, False) == 0
    crlf = fastq_text([b"ACGT", b"GG"], b"\r\n")
    assert cut(crlf, True, False) == len(crlf) and cut(crlf[:-1], True, False) == len(fastq_text([b"ACGT"], b"\r\n")) and cut(b"", True, False) == 0
    quality_at = b"@a\nAC\n+\n@I\n@b\nGT\n+\n@@\n"          # '@' as a quality character never starts a record: lines are counted, not looked at
    assert cut(quality_at, True, False) == len(quality_at) and cut(quality_at[:-3], True, False) == 11


def test_bloom_from_reads_and_spectrum_text(tmp_path):
    config = {"k": K, "m": 1000, "h": 3}
    table = R.count(READS, K)[0]
    path = str(tmp_path / "reads.fastq")
    open(path, "wb").write(fastq_text(READS[:6]))
    spectra = []
    row = kmercount.bloom_from_reads(config, [path] + READS[6:], 2, library="cpu", spectrum_out=spectra)
    assert row.tobytes() == cpu_bloom(R.kept(table, K, 2), K, 1000, 3) and spectra[0].tolist() == R.spectrum(table)
    text = kmercount.spectrum_text(spectra[0])
    lines = text.split("\n")
    assert len(lines) == 257 and lines[-1] == "" and lines[0] == "0\t0" and [l.split("\t") for l in lines[:-1]] == [[str(c), str(n)] for c, n in enumerate(R.spectrum(table))]
    from bigsi_amd.graph.bigsi import BIGSI
    for bad, kw, err in (("ACGT", {}, TypeError), (b"ACGT", {}, TypeError), ([b"ACGT"], {"min_count": 0}, ValueError), ([b"ACGT"], {"min_count": 1.5}, TypeError)):
        with pytest.raises(err):
            BIGSI.bloom_from_reads(config, bad, **kw)
    with pytest.raises(ValueError, match=r"k in \[1, 32\]"):
        BIGSI.bloom_from_reads({"k": 33, "m": 1000, "h": 3}, [b"ACGT"])


class _Refused(Exception):
    pass


class _Parser(object):
    def error(self, msg):
        raise _Refused(msg)


def test_bloom_command_routes_and_refusals(tmp_path, capsys):
    from bigsi_amd.__main__ import bloom_counter_route, bloom_input_head, build_parser, main
    p = build_parser()[0]
    a = p.parse_args(["bloom", "in.fastq", "out.bloom", "-c", "c.yaml"])
    assert (a.min_count, a.spectrum) == (None, None)
    a = p.parse_args(["bloom", "in.fastq", "out.bloom", "--min-count", "2", "--spectrum", "s.tsv"])
    assert (a.min_count, a.spectrum) == (2, "s.tsv")
    with pytest.raises(SystemExit):
        p.parse_args(["bloom", "in.fastq", "out.bloom", "--min-count", "two"])
    route = lambda first, mc=None, sp=None, k=31: bloom_counter_route(_Parser(), first, mc, sp, k)
    # FASTQ always goes to the counter, FASTA only when asked; a Cortex graph and a list take the routes of before
    assert route(b"@r1\nAC") == 1 and route(b"@r1\nAC", 3) == 3 and route(b"@r1\nAC", None, "s.tsv") == 1
    assert route(b">s\nACG") is None and route(b">s\nACG", 1) == 1 and route(b">s\nACG", None, "s.tsv") == 1 and route(b">s\nACG", 2, "s.tsv") == 2
    assert route(b"CORTEX") is None and route(b"ACGTAC") is None and route(b"") is None
    assert route(b">s\nACG", k=63) is None and route(b"CORTEX", k=63) is None          # today's routes have no bound on k
    for first, mc, sp, k, words in ((b"@r1\nAC", None, None, 33, "k <= 32"), (b">s\nACG", 2, None, 33, "k <= 32"), (b">s\nACG", None, "s", 63, "k <= 32"),
                                    (b"@r1\nAC", 0, None, 31, "at least 1"), (b">s\nACG", -3, None, 31, "at least 1"), (b"CORTEX", 0, None, 31, "at least 1"),
                                    (b"CORTEX", 2, None, 31, "Cortex graph"), (b"ACGTAC", 2, None, 31, "k-mer list"), (b"ACGTAC", None, "s", 31, "k-mer list")):
        with pytest.raises(_Refused, match=words):
            route(first, mc, sp, k)
    gz = str(tmp_path / "r.fastq.gz")
    with gzip.open(gz, "wb") as f:
        f.write(fastq_text(READS))
    plain = str(tmp_path / "r.fasta")
    open(plain, "wb").write(fasta_text(READS))
    assert bloom_input_head(gz) == b"@r0 so" and bloom_input_head(plain) == b">s0\nAC"
    # a gzip file is looked into for the counter only: gzipped FASTA without the options, and gzipped anything else, keep the route
    # their own bytes gave them before (the k-mer list route)
    fa_gz, list_gz = str(tmp_path / "r.fasta.gz"), str(tmp_path / "kmers.txt.gz")
    with gzip.open(fa_gz, "wb") as f:
        f.write(fasta_text(READS))
    with gzip.open(list_gz, "wb") as f:
        f.write(b"ACGTACG\nCORTEX\n")
    assert bloom_input_head(fa_gz)[:2] == b"\x1f\x8b" and route(bloom_input_head(fa_gz)) is None and bloom_input_head(fa_gz, True) == b">s0\nAC"
    assert bloom_input_head(list_gz, True)[:2] == b"\x1f\x8b" == bloom_input_head(list_gz)[:2]
    # the whole command: refused with a clean message before anything touches a device (there is none here)
    config = str(tmp_path / "c.yaml")
    open(config, "w").write("h: 3\nk: 33\nm: 1000\nstorage-engine: hip-hbm\nstorage-config:\n  name: none\n")
    fq = str(tmp_path / "r.fastq")
    open(fq, "wb").write(fastq_text(READS))
    out = str(tmp_path / "out.bloom")
    for argv, words in ((["bloom", fq, out, "-c", config], "k <= 32"), (["bloom", plain, out, "-c", config, "--min-count", "0"], "at least 1")):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and words in capsys.readouterr().err and not os.path.exists(out)


def test_bloom_command_writes_filter_and_spectrum(tmp_path, monkeypatch):
    """The command's counter route from the arguments to the two files, with the counter bound to the host twin (the device route is
    tests/test_gpu_kmercount_cli.py's)."""
    import functools
    from bigsi_amd.__main__ import main
    monkeypatch.setattr(kmercount, "bloom_from_reads", functools.partial(kmercount.bloom_from_reads, library="cpu"))
    table = R.count(READS, K)[0]
    config = str(tmp_path / "c.yaml")
    open(config, "w").write("h: 3\nk: %d\nm: 1000\nstorage-engine: hip-hbm\nstorage-config:\n  name: none\n" % K)
    for name, text, argv, mc in (("r.fastq", fastq_text(READS), [], 1), ("r.fastq.gz", fastq_text(READS, b"\r\n"), ["--min-count", "2"], 2),
                                 ("r.fasta", fasta_text(READS), ["--min-count", "3"], 3), ("s.fasta", fasta_text(READS), ["--spectrum", str(tmp_path / "only.tsv")], 1)):
        path, out, spec = str(tmp_path / name), str(tmp_path / (name + ".bloom")), str(tmp_path / (name + ".tsv"))
        with (gzip.open if name.endswith(".gz") else open)(path, "wb") as f:
            f.write(text)
        argv = argv if "--spectrum" in argv else argv + ["--spectrum", spec]
        assert main(["bloom", path, out, "-c", config] + argv) == 0
        assert open(out, "rb").read() == cpu_bloom(R.kept(table, K, mc), K, 1000, 3)
        assert open(argv[argv.index("--spectrum") + 1]).read() == kmercount.spectrum_text(R.spectrum(table))


def test_abi_lists_the_new_entry_points():
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    src = strip("bigsi_hip_kmercount.h")
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.KMERCOUNT_SIGNATURES) == ["bigsi_hip_kmer_counter_" + n for n in ("add", "bloom", "create", "destroy", "fetch", "info", "reset", "spectrum")]
    twin = strip("bigsi_cpu_kmercount.h")
    proto = lambda text, prefix: sorted(re.sub(r"\s+", " ", m).replace(prefix, "X") for m in re.findall(r"int %s_kmer_counter_\w+\([^;]*\);" % prefix, text))
    assert proto(src, "bigsi_hip") == proto(twin, "bigsi_cpu") and len(proto(src, "bigsi_hip")) == 8          # one shape, two libraries
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.KMERCOUNT_SIGNATURES[name][1] and _lib.KMERCOUNT_SIGNATURES[name][0] is C.c_int
        assert name not in _lib.SIGNATURES and name not in strip("bigsi_hip.h")
    assert "bigsi_hip_kmer_counter_set_limits(" in strip("bigsi_hip_testing.h") and _lib.SIGNATURES["bigsi_hip_kmer_counter_set_limits"][1] == [C.c_void_p, C.c_uint64, C.c_uint64]
    assert "no counterpart" not in open(os.path.join(ROOT, "include", "bigsi_cpu_kmercount.h")).read()
