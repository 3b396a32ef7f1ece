"""Column compaction on the device: bigsi_hip_compact_columns / bigsi_hip_extract_columns (k_compact_columns) and
bigsi_hip_shrink_to_fit against numpy on the very bits written with set_rows -- expected = packbits(bits[:, keep]), bit-exact, read
back at the old row width and at the full stride so that the freed tail and the padding are seen to be zero -- and BIGSI.vacuum /
BIGSI.extract and the `vacuum` / `extract` commands on top of it.  Every column of the matrices differs from its neighbours, so a
column that lands in the wrong place shows.  The kernel walks a row in chunks of 64 destination words (4096 columns) whatever the
width, a wavefront owns 8 rows at a time and the grid strides over the row groups: the shapes cross each of those."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import ROOT
from raw_index import Raw, ptr, ragged_bits, rand_seq
from test_compact_columns_host import WIDTHS, expected_rows, keep_patterns, pack_keep

pytestmark = pytest.mark.gpu
_counter = itertools.count()
ERR_INVALID, ERR_STATE = -1, -6


def compact(a, keep, handle=None):
    kept = C.c_uint64(1 << 60)
    return a.L.bigsi_hip_compact_columns(handle or a.ix, ptr(keep), C.byref(kept)), kept.value


def check_compact_and_extract(bits, flags, keep, ctx):
    """In place and out of place give numpy's rows, zero from column K to the end of the stride; the source of an extraction stays."""
    m, n = bits.shape
    k = int(flags.sum())
    a, src, dst = Raw.from_bits(bits), Raw.from_bits(bits), Raw(m=m, n=0, cap=1)
    try:
        before = src.rows()
        rc, kept = compact(a, keep)
        assert rc == 0 and kept == k == a.info().num_cols, ctx
        for rb in ((n + 7) // 8, None):
            got = a.rows(row_bytes=rb)
            assert np.array_equal(got, expected_rows(bits, flags, got.shape[1])), ctx
        assert a.L.bigsi_hip_extract_columns(dst.ix, src.ix, ptr(keep)) == 0, a.L.bigsi_hip_last_error()
        assert dst.info().num_cols == k and dst.info().col_capacity >= k, ctx
        got = dst.rows()
        assert np.array_equal(got, expected_rows(bits, flags, got.shape[1])), ctx
        assert np.array_equal(src.rows(), before) and src.info().num_cols == n, ctx
    finally:
        for r in (a, src, dst):
            r.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_a_widths_and_keep_patterns(n):
    bits = ragged_bits(257, n)
    for label, flags, keep in keep_patterns(n):
        check_compact_and_extract(bits, flags, keep, (n, label))


@pytest.mark.parametrize("density", [0.9, 0.02])
def test_b_rows_far_wider_than_a_chunk(density):
    """600 001 columns are 9376 words: 147 chunks of the kernel's 64 destination words at density 0.9 (the last one partial), 3 at 0.02,
    where a destination word draws on ~50 source words; 37 rows are four full row groups of 8 and one of 5."""
    rng = np.random.default_rng(int(density * 100))
    m, n = 37, 600001
    bits = (rng.random((m, n)) < 0.5).astype(np.uint8)
    flags = rng.random(n) < density
    check_compact_and_extract(bits, flags, pack_keep(flags), density)


@pytest.mark.parametrize("m", [1, 2, 4099])
def test_c_row_counts_around_the_grid(m):
    """One row and two (a single partly filled row group), and 4099 rows: 513 row groups on 129 workgroups' wavefronts."""
    n = 1000
    bits = ragged_bits(m, n) if m > 2 else (np.random.default_rng(m).random((m, n)) < 0.5).astype(np.uint8)
    for label, flags, keep in keep_patterns(n)[-4:]:
        check_compact_and_extract(bits, flags, keep, (m, label))


def test_d_views_and_refusals():
    rng = np.random.default_rng(4)
    bits = ragged_bits(300, 200)
    flags = rng.random(200) < 0.5
    keep = pack_keep(flags)
    a, dst = Raw.from_bits(bits), Raw(m=300, n=0, cap=1)
    view = C.c_void_p()
    a.lib.check(a.L.bigsi_hip_open_view(a.ix, C.byref(view)))
    try:
        before = a.rows()
        # a view is read-only, and its owner does not compact under it
        for handle in (view, a.ix):
            rc, _ = compact(a, keep, handle)
            assert rc == ERR_STATE and a.L.bigsi_hip_last_error()
        assert np.array_equal(a.rows(), before) and a.info().num_cols == 200 == a.info(view).num_cols
        # an empty destination with a view of its own open is refused: the view's column count would go stale
        dst_view = C.c_void_p()
        a.lib.check(a.L.bigsi_hip_open_view(dst.ix, C.byref(dst_view)))
        try:
            assert a.L.bigsi_hip_extract_columns(dst.ix, a.ix, ptr(keep)) == ERR_STATE and b"view" in a.L.bigsi_hip_last_error()
            assert dst.info().num_cols == 0 and not dst.rows().any()
        finally:
            a.lib.check(a.L.bigsi_hip_close(dst_view))
        # ... but a view is a fine source
        assert a.L.bigsi_hip_extract_columns(dst.ix, view, ptr(keep)) == 0, a.L.bigsi_hip_last_error()
        got = dst.rows()
        assert np.array_equal(got, expected_rows(bits, flags, got.shape[1])) and dst.info().num_cols == int(flags.sum())
        assert a.L.bigsi_hip_extract_columns(view, dst.ix, ptr(keep)) == ERR_STATE          # ... and no destination
    finally:
        a.lib.check(a.L.bigsi_hip_close(view))
    try:
        rc, kept = compact(a, keep)                                                          # the view is closed: now it goes
        assert rc == 0 and kept == int(flags.sum())
        assert np.array_equal(a.rows(), dst.rows()[:, :a.rows().shape[1]])
    finally:
        a.close()
        dst.close()


def test_e_capacity_with_slack():
    """Opened for 5000 columns, holding 1000: everything from column K to the end of the 640-byte stride is zero afterwards."""
    bits = ragged_bits(100, 1000)
    flags = np.random.default_rng(5).random(1000) < 0.7
    a = Raw.from_bits(bits, cap=5000)
    try:
        stride = int(a.info().row_stride_bytes)
        assert stride == 640
        rc, kept = compact(a, pack_keep(flags))
        assert rc == 0 and kept == int(flags.sum())
        assert a.info().row_stride_bytes == stride and a.info().col_capacity == 5120          # stride and capacity unchanged
        assert np.array_equal(a.rows(), expected_rows(bits, flags, stride))
    finally:
        a.close()


def test_f_shrink_to_fit():
    bits = ragged_bits(300, 3000)
    flags = np.zeros(3000, bool)
    flags[::7] = True
    a = Raw.from_bits(bits)
    try:
        assert a.L.bigsi_hip_shrink_to_fit(a.ix) == 0 and a.info().row_stride_bytes == 384          # already minimal: a no-op
        rc, kept = compact(a, pack_keep(flags))
        assert rc == 0 and kept == 429
        old = a.info()
        view = C.c_void_p()
        a.lib.check(a.L.bigsi_hip_open_view(a.ix, C.byref(view)))
        assert a.L.bigsi_hip_shrink_to_fit(a.ix) == ERR_STATE and a.L.bigsi_hip_last_error()          # refused with views open
        assert a.L.bigsi_hip_shrink_to_fit(view) == ERR_STATE
        a.lib.check(a.L.bigsi_hip_close(view))
        assert a.info().row_stride_bytes == old.row_stride_bytes
        assert a.L.bigsi_hip_shrink_to_fit(a.ix) == 0, a.L.bigsi_hip_last_error()
        new = a.info()
        assert new.row_stride_bytes == 128 and new.col_capacity == 1024 and new.num_cols == 429          # stride_for(429): 16 words
        assert new.index_bytes == 300 * 128 < old.index_bytes
        assert np.array_equal(a.rows(), expected_rows(bits, flags, 128))
        assert a.L.bigsi_hip_shrink_to_fit(a.ix) == 0 and a.info().row_stride_bytes == 128          # a second call is a no-op
        rc, kept = compact(a, pack_keep(np.zeros(429, bool)))                                         # nothing kept, then shrunk
        assert rc == 0 and kept == 0 and a.L.bigsi_hip_shrink_to_fit(a.ix) == 0 and a.info().row_stride_bytes == 128
        assert not a.rows().any()
    finally:
        a.close()


def test_g_errors():
    bits = ragged_bits(64, 100)
    keep = pack_keep(np.ones(100, bool))
    a, full, other, empty = Raw.from_bits(bits), Raw.from_bits(bits), Raw(m=65, n=0, cap=1), Raw(m=64, n=0, cap=1)
    L = a.L
    try:
        for rc, want in ((L.bigsi_hip_compact_columns(None, ptr(keep), None), ERR_INVALID),
                         (L.bigsi_hip_compact_columns(a.ix, None, None), ERR_INVALID),
                         (L.bigsi_hip_extract_columns(None, a.ix, ptr(keep)), ERR_INVALID),
                         (L.bigsi_hip_extract_columns(empty.ix, None, ptr(keep)), ERR_INVALID),
                         (L.bigsi_hip_extract_columns(empty.ix, a.ix, None), ERR_INVALID),
                         (L.bigsi_hip_extract_columns(a.ix, a.ix, ptr(keep)), ERR_INVALID),             # dst == src
                         (L.bigsi_hip_extract_columns(other.ix, a.ix, ptr(keep)), ERR_INVALID),         # differing m
                         (L.bigsi_hip_extract_columns(full.ix, a.ix, ptr(keep)), ERR_STATE),            # non-empty dst
                         (L.bigsi_hip_shrink_to_fit(None), ERR_INVALID)):
            assert rc == want and L.bigsi_hip_last_error()
        assert L.bigsi_hip_compact_columns(a.ix, ptr(keep), None) == 0                                  # new_num_cols may be NULL
        for r in (a, full):
            assert np.array_equal(r.rows(row_bytes=13), np.packbits(bits, axis=1)) and r.info().num_cols == 100  # nothing changed anything
        assert empty.info().num_cols == 0 and not empty.rows().any()
    finally:
        for r in (a, full, other, empty):
            r.close()


# --------------------------------------------------------------------------------------------- BIGSI level
K, M, H, N_SAMPLES = 11, 4099, 3, 70
DEAD = (0, 63, 64, 69, 30)


def config(d, tag):
    return {"storage-engine": "hip-hbm", "k": K, "m": M, "h": H, "storage-config": {"name": "%s%d" % (tag, next(_counter)), "filename": str(d / ("%s.hbm" % tag))}}


def state_of(b):
    """(every host-side record, every row at the full stride) of an index."""
    st = b.storage
    rows = st.res.get_rows(np.arange(M, dtype=np.uint64), int(st.res.info().row_stride_bytes))
    return {k: st[k] for k in st.record_keys()}, np.asarray(rows)


def searches(b, queries):
    return [b.search(queries[0]), b.search(queries[1], 0.4), b.search(queries[0], score=True), b.search(queries[1], 0.4, score=True),
            b.search(queries[1], 0.4, limit=3), b.sample_stats()]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """70 samples (the colours cross a 64-column word), each a mutated copy of one base sequence so that a query has many partial
    hits; their Bloom filters from BIGSI.bloom are what a fresh build is made of."""
    from bigsi_amd import BIGSI
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(77)
    base = rand_seq(rng, 240)
    seqs = {}
    for c in range(N_SAMPLES):
        cut = int(rng.integers(60, 200))
        seqs["s%d" % c] = base[:cut] + rand_seq(rng, 240 - cut)
    d = tmp_path_factory.mktemp("compact")
    cfg = config(d, "main")
    b = BIGSI.build_from_sequences(cfg, {n: [s] for n, s in seqs.items()})
    filters = {n: BIGSI.bloom(cfg, list(seq_to_kmers(s, K))) for n, s in seqs.items()}
    queries = [base[:100], base[:200]]
    made = [b]
    yield {"b": b, "cfg": cfg, "dir": d, "seqs": seqs, "filters": filters, "queries": queries, "made": made}
    for x in made:
        x.delete()


def test_h_extract_a_subset(world):
    from bigsi_amd import BIGSI
    b, d = world["b"], world["dir"]
    picked = ["s66", "s5", "s64", "s2", "s63"]
    in_order = sorted(picked, key=lambda n: int(n[1:]))
    sub = b.extract(config(d, "sub"), picked)
    fresh = BIGSI.build(config(d, "subfresh"), [world["filters"][n] for n in in_order], in_order)
    world["made"] += [sub, fresh]
    assert sub.num_samples == 5 and [sub.colour_to_sample(c) for c in range(5)] == in_order
    (kv1, rows1), (kv2, rows2) = state_of(sub), state_of(fresh)
    assert kv1 == kv2 and np.array_equal(rows1, rows2)
    assert searches(sub, world["queries"]) == searches(fresh, world["queries"])
    assert b.num_samples == N_SAMPLES                                    # the source is as it was
    for bad, err in ((["nobody"], KeyError), ([], ValueError), (["s1", "s1"], ValueError)):
        with pytest.raises(err):
            b.extract(config(d, "never"), bad)
    with pytest.raises(ValueError):
        b.extract(dict(config(d, "never"), m=M + 1), ["s1"])


def test_i_vacuum_equals_a_fresh_build(world):
    from bigsi_amd import BIGSI
    b, d, q = world["b"], world["dir"], world["queries"]
    assert b.vacuum() == 0                                               # nothing deleted: nothing to do
    for c in DEAD:
        b.delete_sample("s%d" % c)
    with pytest.raises(KeyError):
        b.extract(config(d, "never"), ["s1", "s63"])                    # a deleted name
    before = [b.search(q[0]), b.search(q[1], 0.4)]
    assert all(len(r) > 3 for r in before)
    old_bytes = int(b.storage.res.info().index_bytes)
    assert b.vacuum(shrink=False) == len(DEAD)
    assert b.num_samples == N_SAMPLES - len(DEAD) == b.storage.res.info().num_cols and b.scorer.DB_SIZE == b.num_samples
    assert int(b.storage.res.info().index_bytes) == old_bytes
    kept = [n for c, n in enumerate(world["seqs"]) if c not in DEAD]
    fresh = BIGSI.build(config(d, "fresh"), [world["filters"][n] for n in kept], kept)
    world["made"].append(fresh)
    (kv1, rows1), (kv2, rows2) = state_of(b), state_of(fresh)
    assert kv1 == kv2 and np.array_equal(rows1, rows2)
    got = searches(b, q)
    assert got == searches(fresh, q)
    # against the index before the vacuum: the same samples with the same k-mers found
    for old, new in zip(before, got[:2]):
        assert [(r["sample_name"], r["num_kmers_found"]) for r in old] == [(r["sample_name"], r["num_kmers_found"]) for r in new]
    assert b.vacuum() == 0
    # a vacuumed name can be inserted again, and is the last colour
    b.insert(world["filters"]["s0"], "s0")
    assert b.sample_to_colour("s0") == N_SAMPLES - len(DEAD) and b.num_samples == N_SAMPLES - len(DEAD) + 1
    hit = [r for r in b.search(world["seqs"]["s0"][:100]) if r["sample_name"] == "s0"]
    assert len(hit) == 1 and hit[0]["percent_kmers_found"] == 100


def test_j_vacuum_with_shrink_and_a_wide_capacity(tmp_path):
    """An index opened for 5000 columns gives the stride back: 640 -> 128 bytes per row."""
    from bigsi_amd import BIGSI
    rng = np.random.default_rng(9)
    cfg = config(tmp_path, "wide")
    cfg["storage-config"]["max_cols"] = 5000
    seqs = {"w%d" % c: [rand_seq(rng, 80)] for c in range(9)}
    b = BIGSI.build_from_sequences(cfg, seqs)
    try:
        assert b.storage.res.info().row_stride_bytes == 640
        want = b.search(seqs["w4"][0][:40])
        b.delete_sample("w8")
        b.delete_sample("w1")
        assert b.vacuum() == 2 and b.storage.res.info().row_stride_bytes == 128
        got = b.search(seqs["w4"][0][:40])
        assert [r["sample_name"] for r in got] == [r["sample_name"] for r in want] == ["w4"]
        assert [b.colour_to_sample(c) for c in range(7)] == ["w0", "w2", "w3", "w4", "w5", "w6", "w7"]
    finally:
        b.delete()


def test_k_groups_are_refused(tmp_path):
    from bigsi_amd import BIGSI
    from bigsi_amd._lib import BigsiHipError
    rng = np.random.default_rng(10)
    cfg = config(tmp_path, "grp")
    cfg["storage-config"].update(devices=[0, 0], max_cols=8)
    del cfg["storage-config"]["filename"]
    b = BIGSI.build_from_sequences(cfg, {"g%d" % c: [rand_seq(rng, 60)] for c in range(6)})
    try:
        b.delete_sample("g2")
        for call in (b.vacuum, lambda: b.extract(config(tmp_path, "never"), ["g1"]), b.storage.shrink_to_fit,
                     lambda: b.storage.compact_columns(np.ones(6, bool))):
            with pytest.raises(BigsiHipError) as e:
                call()
            assert e.value.code == ERR_STATE
        assert b.num_samples == 6 and b.sample_to_colour("g3") == 3          # nothing was renumbered
    finally:
        b.delete()


def test_l_cli_vacuum_and_extract(tmp_path, capsys):
    """`python -m bigsi_amd vacuum` / `extract` in processes of their own on an index's snapshot, each followed by a `search` (through the
    same main(), on the snapshot the child left) that sees the new colours."""
    from bigsi_amd import BIGSI
    from bigsi_amd.__main__ import main
    from bigsi_amd.storage.hip_hbm import HipHbmStorage
    rng = np.random.default_rng(11)
    cfg, to = config(tmp_path, "cli"), config(tmp_path, "clito")
    seqs = {"c%d" % c: [rand_seq(rng, 90)] for c in range(7)}
    b = BIGSI.build_from_sequences(cfg, seqs)
    b.delete_sample("c0")
    b.delete_sample("c4")
    b.storage.sync()
    HipHbmStorage.drop(cfg["storage-config"]["name"])                     # (the snapshot is what the child processes see)
    cf, tf = tmp_path / "config.yaml", tmp_path / "to.yaml"
    cf.write_text(yaml.safe_dump(cfg))
    tf.write_text(yaml.safe_dump(to))

    def child(*argv):
        r = subprocess.run([sys.executable, "-m", "bigsi_amd"] + list(argv), cwd=str(tmp_path), capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    def here(*argv):
        capsys.readouterr()
        assert main(list(argv)) == 0
        return json.loads(capsys.readouterr().out)

    out = child("vacuum", "--config", str(cf))
    assert out == json.dumps({"result": "removed 2 of 7 samples", "removed": 2, "num_samples": 5}) + "\n"
    try:
        got = here("search", seqs["c5"][0][:50], "--config", str(cf))
        assert [r["sample_name"] for r in got["results"]] == ["c5"]
        assert here("vacuum", "--config", str(cf), "--no-shrink") == {"result": "removed 0 of 5 samples", "removed": 0, "num_samples": 5}
        assert [BIGSI(cfg).colour_to_sample(c) for c in range(5)] == ["c1", "c2", "c3", "c5", "c6"]
        out = json.loads(child("extract", str(tf), "-s", "c6", "-s", "c2", "--config", str(cf)))
        assert out == {"result": "extracted 2 of 5 samples from %s into %s." % (cf, tf), "num_samples": 2}
        got = here("search", seqs["c6"][0][:50], "--config", str(tf))
        assert [r["sample_name"] for r in got["results"]] == ["c6"]
        sub = BIGSI(to)
        assert [sub.colour_to_sample(c) for c in range(sub.num_samples)] == ["c2", "c6"]
    finally:
        for c in (to, cfg):
            get = BIGSI(c) if os.path.exists(c["storage-config"]["filename"]) else None
            if get is not None:
                get.delete()
