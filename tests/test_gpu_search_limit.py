"""Ranked top-N search: search(seq, threshold, score, limit=N) == search(seq, threshold, score)[:N] on every route -- search (the
sliced small-batch route), search_batch (thousands of queries, one slice), search_stream (several device batches in flight, the
streaming call and the scored batch route), the non-ASCII element batches, a device group and the CLI -- with the device selecting
the N hits (k_rank_select): ties at the cutoff to the lowest colours, deleted samples skipped before the cut, one- and multi-digit
selections, 16- and 32-bit counters.  The unlimited results themselves are pinned against the oracle by test_gpu_parity.py;
here they are the yardstick, and the batch-level checks compare with the oracle's counts directly."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import ROOT, assert_results_equal
from raw_index import rand_seq

pytestmark = pytest.mark.gpu
_counter = itertools.count()
K = 31
LIMITS = (1, 7, 64, 10 ** 9)
THRESHOLDS = (1.0, 0.0, 0.29, 0.4, 0.83)


def cfg(m, h=3, **sc):
    sc.setdefault("name", "lim%d" % next(_counter))
    return {"storage-engine": "hip-hbm", "storage-config": sc, "k": K, "m": m, "h": h}


def topn_colours(colours, counts, n, exact):
    """The reference's order (ascending colour; thresholded: stable sort by count, descending) cut to n, back in ascending colour."""
    colours, counts = np.asarray(colours), np.asarray(counts)
    order = np.arange(colours.size) if exact else np.lexsort((colours, -counts.astype(np.int64)))
    return np.sort(colours[order[:n]])


@pytest.fixture(scope="module")
def ranked():
    """An index whose samples hold prefixes of two queries of very different lengths (a wide spread of counts), blocks of identical
    samples (ties across every cutoff), and unrelated samples; plus reads drawn from the first query."""
    from bigsi_amd import BIGSI
    rng = np.random.default_rng(2024)
    q = rand_seq(rng, 1000)
    gene = rand_seq(rng, 6000)
    samples = {}
    for j in range(120):
        samples["p%03d" % j] = [q[: 31 + (j * 7919) % 970]]           # counts spread over 1 .. 970
    for j in range(40):
        samples["tie%02d" % j] = [q[:500]]                            # 40 identical samples
    for j in range(60):
        samples["g%02d" % j] = [gene[: 31 + (j * 104729) % 5970]]     # counts spread over 1 .. 5970
    for j in range(30):
        samples["r%02d" % j] = [rand_seq(rng, 400)]
    c = cfg(400009)
    b = BIGSI.build_from_sequences(c, samples)
    reads = [q[a: a + 100] for a in rng.integers(0, 900, size=3000)] + [rand_seq(rng, 100) for _ in range(200)]
    yield b, q, gene, reads
    b.delete()


def test_equivalence_search_single_query(ranked):
    b, q, gene, _ = ranked
    for seq in (q, q[:200]):
        for t in THRESHOLDS:
            for score in (False, True):
                full = b.search(seq, t, score)
                for n in LIMITS:
                    assert_results_equal(b.search(seq, t, score, limit=n), full[:n], "search t=%r score=%r n=%d" % (t, score, n))


def test_equivalence_search_batch_many_queries(ranked):
    b, q, gene, reads = ranked
    for t in THRESHOLDS:
        full = b.search_batch(reads, t, False)
        for n in LIMITS:
            got = b.search_batch(reads, t, False, limit=n)
            for i in range(0, len(reads), 37):
                assert_results_equal(got[i], full[i][:n], "batch t=%r n=%d query %d" % (t, n, i))
            assert all(len(g) == min(n, len(f)) for g, f in zip(got, full))
    sub = reads[:300]
    for t in (1.0, 0.4):
        full = b.search_batch(sub, t, True)
        for n in (1, 7):
            got = b.search_batch(sub, t, True, limit=n)
            for g, f in zip(got, full):
                assert_results_equal(g, f[:n], "scored batch t=%r n=%d" % (t, n))


def test_equivalence_search_stream(ranked):
    b, q, gene, reads = ranked
    seqs = reads[:1500] + [q, gene[:1200]]
    for t in (1.0, 0.4, 0.0):
        for score in (False, True):
            full = b.search_batch(seqs, t, score) if score else [r for _, r in b.search_stream(seqs, t, False, batch_size=64)]
            for n in (1, 7, 10 ** 9):
                got = list(b.search_stream(seqs, t, score, batch_size=64, limit=n))
                assert [s for s, _ in got] == seqs
                for i, (_, r) in enumerate(got):
                    if score and i % 11:
                        continue
                    assert_results_equal(r, full[i][:n], "stream t=%r score=%r n=%d query %d" % (t, score, n, i))


def test_against_oracle_counts_every_route(ranked):
    """Batch level, against the oracle: the hit lists of a limited run are the reference's first N, from the oracle's per-sample
    counts (sliced single query, one-slice batch, 32-bit counters below)."""
    from bigsi_amd.storage import get_storage
    from oracle.ref_model import SynthOracle
    m, n_cols, h, seed = 20011, 3000, 3, 99
    st = get_storage(cfg(m, h, max_cols=n_cols))
    st.delete_all()
    for key, v in (("number_of_rows", m), ("number_of_cols", n_cols), ("ksi:bloomfilter_size", m), ("ksi:num_hashes", h)):
        st.set_integer(key, v)
    st.fill_synthetic(seed, 0, 2)
    orc = SynthOracle(seed, 0, m, n_cols, h, K, 2)
    rng = np.random.default_rng(5)
    for seqs in ([rand_seq(rng, 400)], [rand_seq(rng, 150) for _ in range(2500)]):
        batch = st.new_batch(seqs, K)
        for t in (1.0, 0.4, 0.0):
            batch.set_limit(7)
            batch.run(t, sparse_counts=True)
            _, nu, mk = batch.unique()
            off, col, cnt = batch.hits()
            for i in range(0, len(seqs), 97):
                u, c = orc.counts(seqs[i])
                hit = np.flatnonzero(c >= (u if t == 1.0 else mk[i]))
                want = topn_colours(hit, c[hit], 7, t == 1.0)
                assert np.array_equal(col[int(off[i]):int(off[i + 1])], want), (t, i)
                assert np.array_equal(cnt[int(off[i]):int(off[i + 1])], c[want])
        batch.close()
    st.delete_all()


def test_ties_at_the_cutoff_go_to_the_lowest_colours(ranked):
    b, q, _, _ = ranked
    names = [r["sample_name"] for r in b.search(q, 0.4)]
    ties = [nm for nm in names if nm.startswith("tie")]
    assert len(ties) == 40
    for n in (3, 25):
        first = names.index("tie00")
        got = [r["sample_name"] for r in b.search(q, 0.4, limit=first + n)]
        assert got[first:] == ["tie%02d" % j for j in range(n)]


def test_multi_digit_selection_gene_length_query(ranked):
    """> 4096 unique k-mers at threshold 0: every sample is a hit, counts spread over 0 .. 5970 -- two 12-bit digits."""
    b, _, gene, _ = ranked
    full = b.search(gene, 0.0)
    assert full[0]["num_kmers"] > 4096 and len({r["num_kmers_found"] for r in full}) > 50
    for n in (1, 7, 64, 100):
        assert_results_equal(b.search(gene, 0.0, limit=n), full[:n], "gene n=%d" % n)
    full = b.search(gene, 0.5, True)
    assert_results_equal(b.search(gene, 0.5, True, limit=5), full[:5], "gene scored")


def test_uint32_counters():
    """> 65 535 k-mers in one query: 32-bit counters.  66 000 k-mers are 17 bits: TWO 12-bit digits (the third pass needs 2^24 unique
    k-mers in one query and is reached through bigsi_hip_rank_select_arrays only: tests/test_gpu_rank_select.py)."""
    from bigsi_amd.storage import get_storage
    from oracle.ref_model import SynthOracle
    m, n_cols, h = 1009, 100, 2
    st = get_storage(cfg(m, h, max_cols=n_cols))
    st.delete_all()
    for key, v in (("number_of_rows", m), ("number_of_cols", n_cols), ("ksi:bloomfilter_size", m), ("ksi:num_hashes", h)):
        st.set_integer(key, v)
    st.fill_synthetic(77, 0, 1)
    orc = SynthOracle(77, 0, m, n_cols, h, K, 1)
    s = rand_seq(np.random.default_rng(3), 66000)
    batch = st.new_batch([s, "ACGT" * 10], K)
    u, c = orc.counts(s)
    for t in (0.0, 0.5):
        batch.set_limit(7)
        batch.run(t, sparse_counts=True)
        assert batch.info().count_bytes == 4
        _, nu, mk = batch.unique()
        off, col, cnt = batch.hits()
        hit = np.flatnonzero(c >= mk[0])
        want = topn_colours(hit, c[hit], 7, False)
        assert np.array_equal(col[:int(off[1])], want) and np.array_equal(cnt[:int(off[1])], c[want]), t
    batch.close()
    st.delete_all()


def test_deleted_samples_are_skipped_and_the_next_fills_in(ranked):
    from bigsi_amd import BIGSI
    _, q, _, _ = ranked
    rng = np.random.default_rng(8)
    samples = {"s%02d" % j: [q[: 100 + 20 * j]] for j in range(20)}
    samples.update({"e%02d" % j: [q[:300]] for j in range(5)})
    b = BIGSI.build_from_sequences(cfg(100003), samples)
    try:
        for t in (1.0, 0.5):
            before = b.search(q[:300], t)
            victim = before[2]["sample_name"]
            b.delete_sample(victim)
            full = b.search(q[:300], t)
            assert victim not in [r["sample_name"] for r in full]
            for n in (1, 3, 5, 10 ** 9):
                got = b.search(q[:300], t, limit=n)
                assert_results_equal(got, full[:n], "deleted t=%r n=%d" % (t, n))
            assert [r["sample_name"] for r in b.search(q[:300], t, limit=3)] == [r["sample_name"] for r in before if r["sample_name"] != victim][:3]
        reads = [q[a: a + 80] for a in rng.integers(0, 200, size=50)]
        for g, f in zip(b.search_batch(reads, 0.5, limit=2), b.search_batch(reads, 0.5)):
            assert_results_equal(g, f[:2], "deleted batch")
    finally:
        b.delete()


def test_limits_that_change_nothing(ranked):
    b, q, _, reads = ranked
    full = b.search(q, 0.4)
    assert_results_equal(b.search(q, 0.4, limit=len(full)), full)
    assert_results_equal(b.search(q, 0.4, limit=len(full) + 1), full)
    # the untrimmed vectors stay fetchable after a limited run
    st = b.storage
    batch = st.new_batch(reads[:20], K)
    batch.run(0.4)
    counts0, off0 = [batch.counts(i) for i in range(20)], batch.hits()[0]
    batch.run(1.0)
    bitmaps0 = [batch.bitmap(i) for i in range(20)]
    batch.set_limit(1)
    batch.run(0.4)
    assert np.array_equal(np.diff(batch.hits()[0].astype(np.int64)), np.minimum(np.diff(off0.astype(np.int64)), 1))
    for i in range(20):
        assert np.array_equal(batch.counts(i), counts0[i])
    batch.run(1.0)
    for i in range(20):
        assert np.array_equal(batch.bitmap(i), bitmaps0[i])
    batch.close()
    # early_exit: the same limited results
    wants = {t: b.search_batch(reads[:200], t, limit=3) for t in (1.0, 0.4)}
    b.config["early_exit"] = True
    try:
        for t in (1.0, 0.4):
            assert b.search_batch(reads[:200], t, limit=3) == wants[t]
    finally:
        b.config.pop("early_exit")


def test_non_ascii_query(ranked):
    b, q, _, _ = ranked
    seq = q[:300] + "αβ" + q[300:400]
    for t in (0.4, 0.0):
        for score in (False, True):
            full = b.search(seq, t, score)
            assert full
            assert_results_equal(b.search(seq, t, score, limit=4), full[:4], "non-ascii t=%r score=%r" % (t, score))


def test_arguments_rejected_before_device_work(ranked):
    b = ranked[0]
    for bad, exc in ((0, ValueError), (-3, ValueError), (True, TypeError), (2.0, TypeError), ("3", TypeError)):
        with pytest.raises(exc):
            b.search("ACGT" * 10, 1.0, limit=bad)
        with pytest.raises(exc):
            b.search_batch(["ACGT" * 10], 1.0, limit=bad)
        with pytest.raises(exc):
            next(b.search_stream(["ACGT" * 10], 1.0, limit=bad))
    # degenerate queries raise the reference's errors exactly as without a limit
    with pytest.raises(TypeError):
        b.search("ACG", 1.0, limit=3)
    with pytest.raises(UnboundLocalError):
        b.search("ACG", 0.5, limit=3)


def test_device_group_uneven_and_empty_shards(ranked):
    """three shards of one device over 250 samples: 128 + 122 + 0 columns (an empty shard); global top N from the shards' top N."""
    from bigsi_amd import BIGSI
    b, q, gene, reads = ranked
    names = [b.colour_to_sample(c) for c in range(b.num_samples)]
    rng = np.random.default_rng(2024)          # (the fixture's samples again)
    assert rand_seq(rng, 1000) == q
    gene2 = rand_seq(rng, 6000)
    samples = {}
    for j in range(120):
        samples["p%03d" % j] = [q[: 31 + (j * 7919) % 970]]
    for j in range(40):
        samples["tie%02d" % j] = [q[:500]]
    for j in range(60):
        samples["g%02d" % j] = [gene2[: 31 + (j * 104729) % 5970]]
    for j in range(30):
        samples["r%02d" % j] = [rand_seq(rng, 400)]
    assert list(samples) == names
    g = BIGSI.build_from_sequences(cfg(400009, devices=[0, 0, 0], max_cols=384), samples)
    try:
        g.delete_sample("tie03")
        b.delete_sample("tie03")
        seqs = reads[:200] + [q, gene[:2000]]
        for t in (1.0, 0.4, 0.0):
            full = b.search_batch(seqs, t)
            for n in (1, 7, 64):
                got = g.search_batch(seqs, t, limit=n)
                for i, (x, y) in enumerate(zip(got, full)):
                    assert_results_equal(x, y[:n], "group t=%r n=%d query %d" % (t, n, i))
    finally:
        g.delete()


def cli(args, cwd, check=True):
    r = subprocess.run([sys.executable, "-m", "bigsi_amd"] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    if check:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def csv_rows(text):
    import csv
    import io
    return [row for row in csv.reader(io.StringIO(text.replace("\r\n", "\n"))) if row and row[0] != "query"]


def test_cli_limit(tmp_path, ranked):
    from bigsi_amd import BIGSI
    from bigsi_amd.frontend import bulk_search, search
    _, q, _, reads = ranked
    c = cfg(100003, filename=str(tmp_path / "index.hbm"))
    samples = {"s%02d" % j: [q[: 60 + 15 * j]] for j in range(30)}
    b = BIGSI.build_from_sequences(c, samples)
    cf = tmp_path / "config.yaml"
    cf.write_text(yaml.safe_dump(c))
    fasta = tmp_path / "q.fasta"
    fasta.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads[:40] + [q[:400]])))
    try:
        want = json.loads(search(b, q[:400], 0.4, False, "json"))
        want["results"] = want["results"][:3]
        out = cli(["search", q[:400], "-t", "0.4", "--limit", "3", "--config", str(cf)], str(tmp_path)).stdout
        assert json.loads(out) == want and out == json.dumps(want, indent=4) + "\n"
        full = json.loads(bulk_search(b, str(fasta), 0.4, False, "json"))
        for rec in full:
            rec["results"] = rec["results"][:3]
        out = cli(["bulk_search", str(fasta), "-t", "0.4", "--limit", "3", "--config", str(cf)], str(tmp_path)).stdout
        assert json.loads(out) == full and out == json.dumps(full, indent=4) + "\n"
        out = cli(["bulk_search", str(fasta), "-t", "0.4", "--limit", "3", "--stream", "--config", str(cf)], str(tmp_path)).stdout
        assert [json.loads(line) for line in out.splitlines() if line.strip()] == full
        per, want_rows = {}, []
        for row in csv_rows(bulk_search(b, str(fasta), 0.4, False, "csv")):
            per[row[0]] = per.get(row[0], 0) + 1
            if per[row[0]] <= 3:
                want_rows.append(row)
        assert len(want_rows) < len(csv_rows(bulk_search(b, str(fasta), 0.4, False, "csv")))
        out = cli(["bulk_search", str(fasta), "-t", "0.4", "--limit", "3", "--format", "csv", "--config", str(cf)], str(tmp_path)).stdout
        assert csv_rows(out) == want_rows
        r = cli(["search", q[:100], "--limit", "3", "--sharded", "--config", str(cf)], str(tmp_path), check=False)
        assert r.returncode == 2 and "--limit" in r.stderr
    finally:
        b.delete()
