"""`python -m bigsi_amd bloom` over raw reads, end to end on the device: a FASTQ file of reads drawn at about 5x coverage from a 2 kb
random genome, some of them with one planted substitution whose k-mers the restatement (tests/kmercount_ref.py) confirms occur once.
`bloom --min-count 2` is BIGSI.bloom of the restatement's kept list, byte for byte, and leaves the errors' k-mers out; a FASTQ input
without the option keeps everything; `bloom --min-count 1` on an ACGT-only FASTA file is the output of `bloom` without the option, byte
for byte; `build` + `search` over the filter finds a window of the genome and not the read that carries an error."""
import itertools
import json

import pytest
import yaml

import kmercount_ref as R

_counter = itertools.count()
K, M, H = 21, 100003, 3
GENOME, READ, N_READS, N_ERRORS = 2000, 100, 100, 8


def revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def sample():
    """(genome, reads, [(read index, error position)]): every eighth read of the first 64 carries one substitution at its middle."""
    rng = R.random.Random(12)
    genome = R.rand_seq(rng, GENOME)
    reads, errors = [], []
    for i in range(N_READS):
        at = rng.randrange(GENOME - READ + 1)
        r = bytearray(genome[at:at + READ])
        if i % 8 == 0 and len(errors) < N_ERRORS:
            p = READ // 2
            r[p] = ord({"A": "C", "C": "G", "G": "T", "T": "A"}[chr(r[p])])
            errors.append((i, p))
        reads.append(revcomp(bytes(r)) if i % 2 else bytes(r))
    return genome, reads, errors


def error_kmers(read, p):
    """The canonical keys of the windows of `read` (as sequenced, forward) that cover position p."""
    return [R.key_of(R.canonical(read[s:s + K])) for s in range(max(p - K + 1, 0), min(p, len(read) - K) + 1)]


def test_the_sample_holds_what_the_checks_need():
    genome, reads, errors = sample()
    table, counted, skipped = R.count(reads, K)
    assert len(errors) == N_ERRORS and skipped == 0 and counted == N_READS * (READ - K + 1)
    for i, p in errors:          # (even reads are forward: the error sits at p)
        keys = error_kmers(reads[i], p)
        assert len(keys) == K and all(table[key] == 1 for key in keys)
    kept2, kept1 = R.kept(table, K, 2), R.kept(table, K, 1)
    assert len(kept1) - len(kept2) >= N_ERRORS * K and len(kept2) > 1000
    assert genome_window(genome, table) is not None


def genome_window(genome, table, length=60):
    """A window of the genome whose k-mers were all seen at least twice."""
    for at in range(0, GENOME - length):
        w = genome[at:at + length]
        if all(table[R.key_of(R.canonical(w[s:s + K]))] >= 2 for s in range(length - K + 1)):
            return w
    return None


@pytest.mark.gpu
def test_bloom_min_count_build_and_search(tmp_path, capsys):
    from bigsi_amd import BIGSI
    from bigsi_amd.__main__ import main
    genome, reads, errors = sample()
    table = R.count(reads, K)[0]
    cfg = {"storage-engine": "hip-hbm", "k": K, "m": M, "h": H, "storage-config": {"name": "kmercount%d" % next(_counter), "filename": str(tmp_path / "index.hbm")}}
    cf, fq, fa = tmp_path / "config.yaml", tmp_path / "reads.fastq", tmp_path / "genome.fasta"
    cf.write_text(yaml.safe_dump(cfg))
    fq.write_bytes(b"".join(b"@read%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads)))
    one, two = genome[:1200], genome[1200:]
    fa.write_bytes(b">genome part one\n" + b"\n".join(one[i:i + 70] for i in range(0, len(one), 70)) + b"\n>part two\n" + two + b"\n")
    out2, out1, spec = tmp_path / "min2.bloom", tmp_path / "min1.bloom", tmp_path / "spectrum.tsv"
    # --min-count 2: the restatement's kept list, and the spectrum beside it
    assert main(["bloom", str(fq), str(out2), "-c", str(cf), "--min-count", "2", "--spectrum", str(spec)]) == 0
    want2 = BIGSI.bloom(cfg, R.kept(table, K, 2))
    assert out2.read_bytes() == want2.tobytes()
    assert spec.read_text() == "".join("%d\t%d\n" % (c, n) for c, n in enumerate(R.spectrum(table)))
    # a FASTQ input without the option: min_count 1, every k-mer of every read
    assert main(["bloom", str(fq), str(out1), "-c", str(cf)]) == 0
    want1 = BIGSI.bloom(cfg, R.kept(table, K, 1))
    assert out1.read_bytes() == want1.tobytes() != want2.tobytes()
    # an ACGT-only FASTA file: --min-count 1 is today's output, byte for byte
    old, new = tmp_path / "fasta_old.bloom", tmp_path / "fasta_new.bloom"
    assert main(["bloom", str(fa), str(old), "-c", str(cf)]) == 0 and main(["bloom", str(fa), str(new), "-c", str(cf), "--min-count", "1"]) == 0
    assert old.read_bytes() == new.read_bytes()
    assert new.read_bytes() == BIGSI.bloom(cfg, R.kept(R.count([one, two], K)[0], K, 1)).tobytes()
    # refused before any device work
    kmers = tmp_path / "kmers.txt"
    kmers.write_text("\n".join(R.kept(table, K, 2)[:5]) + "\n")
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        main(["bloom", str(kmers), str(tmp_path / "never.bloom"), "-c", str(cf), "--min-count", "2"])
    assert e.value.code == 2 and "k-mer list" in capsys.readouterr().err and not (tmp_path / "never.bloom").exists()
    # build + search: the filter answers for the genome and not for a read's error
    assert main(["build", "-b", str(out2), "-s", "sample2", "-c", str(cf)]) == 0
    try:
        capsys.readouterr()
        window = genome_window(genome, table)
        assert main(["search", window.decode(), "-c", str(cf)]) == 0
        found = json.loads(capsys.readouterr().out)
        assert "sample2" in json.dumps(found)
        i, p = errors[0]
        assert main(["search", reads[i].decode(), "-c", str(cf)]) == 0
        assert "sample2" not in capsys.readouterr().out
        # ... while the filter that keeps everything answers for that read too
        assert main(["insert", str(out1), "sample1", "-c", str(cf)]) == 0
        capsys.readouterr()
        assert main(["search", reads[i].decode(), "-c", str(cf)]) == 0
        text = capsys.readouterr().out
        assert "sample1" in text and "sample2" not in text
    finally:
        BIGSI(cfg).delete()
