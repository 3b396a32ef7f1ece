"""Pairwise popcounts on the GPU: bigsi_hip_pairwise_popcounts on the C ABI against numpy on the very bits written
(bits[:, A].T @ bits[:, B], bit-exact in uint64) -- row counts around the 64-row word and the planner's chunk and slice cuts (read
from the compiled planner), selection sizes around the tile edge, where the selected columns lie, counts past 16 bits, symmetry,
stale rows behind num_rows, read-only handles, refusals -- and BIGSI.sample_distances / cluster_samples and the `cluster` and
`collapse` commands end to end on a small built index with planted families."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import yaml

from raw_index import Raw, ptr, rand_seq
from test_pairwise_host import ERR_CAPACITY, ERR_INVALID, ERR_RANGE, SENTINEL, constants, expected, plan, plan_lib, selections  # noqa: F401 (plan_lib: a fixture)

pytestmark = pytest.mark.gpu
_counter = itertools.count()


def pattern_bits(m, n):
    """column c set in the rows r < (c * 37) % 258: heights that differ from column to column within a byte"""
    return (np.arange(m)[:, None] < ((np.arange(n) * 37) % 258)[None, :]).astype(np.uint8)


def pairwise(raw, a, b=None, handle=None, capacity=None, out=None):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.uint32)
    if out is None:
        out = np.full((a.size, a.size if b is None else b.size), SENTINEL, np.uint64)
    rc = raw.L.bigsi_hip_pairwise_popcounts(handle or raw.ix, ptr(a), a.size, ptr(b), 0 if b is None else b.size, ptr(out), out.size if capacity is None else capacity)
    return rc, out


def check(raw, bits, a, b=None, ctx=None):
    rc, out = pairwise(raw, a, b)
    assert rc == 0, (ctx, raw.err())
    assert np.array_equal(out, expected(bits, a, b)), ctx


@pytest.fixture(scope="module")
def row_counts(plan_lib):
    """1 .. 1009 as the issue lists them, then the planner's own cuts for a 200-column index (16 words of stride) and the selections
    below: the row count from which chunks are cut, and the ends of the first chunk and of the first slice of a larger index, each
    -1, 0, +1; 4100 rows make three chunks."""
    k = constants(plan_lib)
    ms = [1, 63, 64, 65, 257, 1009, 4100]
    split = k["split_words"] * 64
    ms += [split - 1 - 63, split - 63, split + 1]          # (the last 64-row word is ragged: 31 words + 1 row is already 32 words)
    for nua in (5, 65):
        p = plan(plan_lib, nua, nua, True, 4100, 16)
        assert p["chunks"] >= 3 and p["slices"] >= 2
        for cut in (p["chunk_words"] * 64, p["slice_words"] * 64, 2 * p["chunk_words"] * 64):
            ms += [cut - 1, cut, cut + 1]
    return sorted(set(ms))


def test_a_rows(row_counts, plan_lib):
    n = 200
    sel = np.array([0, 199, 64, 63, 7, 130], np.uint32)
    wide = np.arange(0, 195, 3, dtype=np.uint32)          # 65 columns: two tiles a side
    full = pattern_bits(max(row_counts), n)
    full[np.arange(full.shape[0]), np.arange(full.shape[0]) % n] ^= 1          # bits in the last rows of every m, too
    for m in row_counts:
        bits = full[:m]
        raw = Raw.from_bits(bits)
        try:
            check(raw, bits, sel, None, ("symmetric", m))
            check(raw, bits, sel[:2], wide, ("rectangular", m))
            if m in (1, 65, 1009, 4100) or m > 2000:
                check(raw, bits, wide, None, ("two tiles", m))
        finally:
            raw.close()


def test_b_selection_sizes_around_the_tile(plan_lib):
    tile = constants(plan_lib)["tile"]
    m, n = 300, 8193
    bits = pattern_bits(m, n)
    rng = np.random.default_rng(3)
    raw = Raw.from_bits(bits)
    try:
        for s in (1, 2, tile - 1, tile, tile + 1, 2 * tile + 1):
            a = rng.permutation(n)[:s].astype(np.uint32)
            b = rng.permutation(n)[:s].astype(np.uint32)
            check(raw, bits, a, None, ("symmetric", s))
            check(raw, bits, a, b[:max(1, s // 2)], ("rectangular", s))
            check(raw, bits, a[:1], b, ("one by many", s))
            check(raw, bits, b, a[:1], ("many by one", s))
        big = rng.permutation(n)[:2500].astype(np.uint32)
        check(raw, bits, big[:1], big, "1 x 2500")
        check(raw, bits, big, big[:1], "2500 x 1")
    finally:
        raw.close()


@pytest.mark.parametrize("n", (65, 129, 8193))
def test_c_column_placement(n):
    m = 300
    bits = pattern_bits(m, n)
    raw = Raw.from_bits(bits)
    try:
        for label, a, b in selections(n):
            check(raw, bits, a, b, (label, n))
    finally:
        raw.close()


def test_d_counts_pass_16_bits():
    m = 70_001
    bits = np.zeros((m, 70), np.uint8)
    bits[:, 3] = bits[:, 66] = 1
    bits[::2, 40] = 1
    raw = Raw.from_bits(bits)
    try:
        rc, out = pairwise(raw, [3, 66, 40])
        assert rc == 0, raw.err()
        assert out.tolist() == [[70_001, 70_001, 35_001], [70_001, 70_001, 35_001], [35_001, 35_001, 35_001]]
        check(raw, bits, [40, 3], [66, 40, 5], "rectangular")
    finally:
        raw.close()


def test_e_symmetry_and_the_diagonal():
    m, n = 2500, 300
    rng = np.random.default_rng(8)
    bits = (rng.random((m, n)) < rng.random(n)[None, :]).astype(np.uint8)
    raw = Raw.from_bits(bits)
    try:
        a = rng.permutation(n)[:150].astype(np.uint32)
        rc, sym = pairwise(raw, a)
        assert rc == 0, raw.err()
        rc, explicit = pairwise(raw, a, a.copy())
        assert rc == 0, raw.err()
        counts = np.zeros(n, np.uint64)
        raw.lib.check(raw.L.bigsi_hip_column_popcounts(raw.ix, None, ptr(counts), n))
        assert np.array_equal(sym, sym.T) and np.array_equal(sym.diagonal(), counts[a]) and np.array_equal(sym, explicit)
        assert np.array_equal(sym, expected(bits, a))
    finally:
        raw.close()


def test_f_stale_rows_behind_num_rows_are_not_counted():
    """an in-place fold leaves the old rows in the allocation until trim_rows"""
    m, n, factor = 3 * 1100, 200, 3
    rng = np.random.default_rng(9)
    bits = (rng.random((m, n)) < 0.3).astype(np.uint8)
    raw = Raw.from_bits(bits)
    try:
        new_m = C.c_uint64(0)
        raw.lib.check(raw.L.bigsi_hip_fold_rows(raw.ix, factor, C.byref(new_m)))
        assert new_m.value == m // factor == int(raw.info().num_rows)
        folded = bits[:1100] | bits[1100:2200] | bits[2200:]
        sel = np.array([199, 0, 64, 63, 100], np.uint32)
        check(raw, folded, sel, None, "folded, not trimmed")
        check(raw, folded, sel[:2], np.arange(0, 200, 3, dtype=np.uint32), "folded, not trimmed, rectangular")
        raw.lib.check(raw.L.bigsi_hip_trim_rows(raw.ix))
        check(raw, folded, sel, None, "trimmed")
    finally:
        raw.close()


def test_g_a_view_reads_what_the_owner_reads():
    bits = pattern_bits(500, 129)
    raw = Raw.from_bits(bits)
    view = C.c_void_p()
    raw.lib.check(raw.L.bigsi_hip_open_view(raw.ix, C.byref(view)))
    try:
        a, b = np.array([128, 0, 64, 63], np.uint32), np.arange(129, dtype=np.uint32)[::-1]
        for bb in (None, b):
            rc1, own = pairwise(raw, a, bb)
            rc2, seen = pairwise(raw, a, bb, handle=view)
            assert rc1 == rc2 == 0, raw.err()
            assert np.array_equal(own, seen) and np.array_equal(own, expected(bits, a, bb))
    finally:
        raw.lib.check(raw.L.bigsi_hip_close(view))
        raw.close()


def test_h_refusals_leave_out_untouched():
    bits = pattern_bits(100, 70)
    raw = Raw.from_bits(bits)
    L = raw.L
    try:
        a, b, bad = np.array([3, 69, 5], np.uint32), np.array([1, 2], np.uint32), np.array([3, 70, 5], np.uint32)
        huge = np.zeros((1 << 14) + 1, np.uint32)
        out = np.full((3, 3), SENTINEL, np.uint64)
        for args, code, says in (((None, 3, None, 0, ptr(out), 9), ERR_INVALID, "NULL"),
                                 ((ptr(a), 3, None, 0, None, 9), ERR_INVALID, "NULL"),
                                 ((ptr(a), 0, None, 0, ptr(out), 9), ERR_INVALID, "empty"),
                                 ((ptr(a), 3, ptr(b), 0, ptr(out), 9), ERR_INVALID, "empty"),
                                 ((ptr(bad), 3, None, 0, ptr(out), 0), ERR_RANGE, "cols_a[1] = 70"),
                                 ((ptr(a), 3, ptr(bad), 3, ptr(out), 0), ERR_RANGE, "cols_b[1] = 70"),
                                 ((ptr(a), 3, None, 0, ptr(out), 8), ERR_CAPACITY, "capacity 8"),
                                 ((ptr(a), 3, ptr(b), 2, ptr(out), 5), ERR_CAPACITY, "capacity 5"),
                                 ((ptr(huge), huge.size, None, 0, ptr(out), 9), ERR_CAPACITY, "capacity 9"),
                                 ((ptr(huge), huge.size, None, 0, ptr(out), 1 << 40), ERR_RANGE, "BIGSI_PAIRWISE_MAX_PAIRS")):
            assert L.bigsi_hip_pairwise_popcounts(raw.ix, *args) == code, (args, raw.err())
            assert says in raw.err().decode(), raw.err()
            assert (out == SENTINEL).all()
        assert L.bigsi_hip_pairwise_popcounts(None, ptr(a), 3, None, 0, ptr(out), 9) == ERR_INVALID
        check(raw, bits, a, b, "after the refusals")          # (and nothing sticks to the handle)
    finally:
        raw.close()


# --------------------------------------------------------------------------------------------- BIGSI level
K, M, H, FAMILIES, N_SAMPLES = 11, 4099, 3, 5, 40


def config(d, tag):
    return {"storage-engine": "hip-hbm", "k": K, "m": M, "h": H, "storage-config": {"name": "pair%s%d" % (tag, next(_counter)), "filename": str(d / ("%s.hbm" % tag))}}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """40 samples in 5 planted families: sample c is family c % 5's base sequence with two point mutations, so that members of a
    family share most of their filters (22 of 290 k-mers differ at most) and families share what chance gives (a Jaccard index
    near 0.1 at this fill)."""
    from bigsi_amd import BIGSI
    rng = np.random.default_rng(41)
    bases = [rand_seq(rng, 300) for _ in range(FAMILIES)]
    seqs = {}
    for c in range(N_SAMPLES):
        s = list(bases[c % FAMILIES])
        for pos in rng.choice(300, 2, replace=False):
            s[pos] = "ACGT"[("ACGT".index(s[pos]) + 1 + int(rng.integers(0, 3))) % 4]
        seqs["s%d" % c] = "".join(s)
    d = tmp_path_factory.mktemp("pairwise")
    cfg = config(d, "main")
    b = BIGSI.build_from_sequences(cfg, {n: [s] for n, s in seqs.items()})
    made = [b]
    yield {"b": b, "cfg": cfg, "dir": d, "seqs": seqs, "bases": bases, "made": made}
    for x in made:
        x.delete()


def families():
    return {"s%d" % f: ["s%d" % c for c in range(f, N_SAMPLES, FAMILIES)] for f in range(FAMILIES)}


def test_i_sample_distances_are_similar_samples_row_by_row(world):
    b = world["b"]
    d = b.sample_distances()
    names = ["s%d" % c for c in range(N_SAMPLES)]
    assert d["samples"] == names == d["against"]
    inter, jac, con = d["bits_shared"], d["jaccard"], d["containment"]
    assert inter.dtype == np.uint64 and inter.shape == jac.shape == con.shape == (N_SAMPLES, N_SAMPLES) and jac.dtype == con.dtype == np.float64
    for i, name in enumerate(names):
        rows = b.similar_samples(name)
        assert sorted(r["colour"] for r in rows) == [c for c in range(N_SAMPLES) if c != i]
        for r in rows:
            c = r["colour"]
            assert (r["sample_name"], r["bits_shared"], r["jaccard"], r["containment"]) == (names[c], int(inter[i, c]), jac[i, c], con[i, c]), (i, c)
    assert (jac.diagonal() == 1.0).all() and (con.diagonal() == 1.0).all()
    # a named selection in its own order, against another: the same numbers
    sub, other = ["s7", "s2", "s39"], ["s0", "s7", "s12", "s2"]
    r = b.sample_distances(sub, other)
    ia, ib = [7, 2, 39], [0, 7, 12, 2]
    assert r["samples"] == sub and r["against"] == other
    assert np.array_equal(r["bits_shared"], inter[np.ix_(ia, ib)]) and np.array_equal(r["jaccard"], jac[np.ix_(ia, ib)]) and np.array_equal(r["containment"], con[np.ix_(ia, ib)])
    for bad, err in ((["nobody"], KeyError), ([], ValueError)):
        with pytest.raises(err):
            b.sample_distances(bad)
        with pytest.raises(err):
            b.sample_distances(None, bad)


def test_j_cluster_recovers_the_families_and_collapse_takes_them(world, capsys):
    """`cluster --out g.tsv`, then `collapse --groups g.tsv`: the groups are the planted families, the collapsed index builds, and
    every exact hit of a member in the full index is a hit of its group in the collapsed one."""
    from bigsi_amd import BIGSI
    from bigsi_amd.__main__ import main
    b, d = world["b"], world["dir"]
    want = families()
    assert b.cluster_samples(0.5) == want and list(b.cluster_samples(0.5)) == list(want)
    some = b.cluster_samples(0.5, ["s11", "s1", "s6", "s3"])
    assert some == {"s1": ["s1", "s6", "s11"], "s3": ["s3"]}
    with pytest.raises(ValueError):
        b.cluster_samples(0.0)
    b.storage.sync()
    to = config(d, "families")
    cf, tf, gf = d / "config.yaml", d / "to.yaml", d / "g.tsv"
    cf.write_text(yaml.safe_dump(world["cfg"]))
    tf.write_text(yaml.safe_dump(to))
    capsys.readouterr()
    assert main(["cluster", "--min-jaccard", "0.5", "--out", str(gf), "--config", str(cf)]) == 0
    assert json.loads(capsys.readouterr().out) == want
    assert main(["collapse", str(tf), "--groups", str(gf), "--config", str(cf)]) == 0
    report = json.loads(capsys.readouterr().out)
    assert report["groups"] == FAMILIES and report["members"] == want and report["samples_dropped"] == 0
    new = BIGSI(to)
    world["made"].append(new)
    assert [new.colour_to_sample(c) for c in range(new.num_samples)] == list(want)
    group_of = {s: g for g, ms in want.items() for s in ms}
    for query in [world["bases"][f][40:120] for f in range(FAMILIES)] + [world["seqs"]["s17"][:90], world["seqs"]["s38"][200:290]]:
        hits = [r["sample_name"] for r in b.search(query)]
        hit_groups = {r["sample_name"] for r in new.search(query)}
        assert hits and all(group_of[s] in hit_groups for s in hits), query
    assert main(["distances", "-s", "s3", "-s", "s8", "--config", str(cf)]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["samples"] == ["s3", "s8"] and out["jaccard"][0][0] == 1.0 and out["jaccard"][0][1] == out["jaccard"][1][0] > 0.5


def test_k_groups_are_refused(tmp_path):
    from bigsi_amd import BIGSI
    from bigsi_amd._lib import ERR_STATE, BigsiHipError
    rng = np.random.default_rng(10)
    cfg = config(tmp_path, "grp")
    cfg["storage-config"].update(devices=[0, 0], max_cols=8)
    del cfg["storage-config"]["filename"]
    b = BIGSI.build_from_sequences(cfg, {"g%d" % c: [rand_seq(rng, 60)] for c in range(6)})
    try:
        for call in (lambda: b.sample_distances(), lambda: b.cluster_samples(0.5), lambda: b.storage.pairwise_popcounts([0, 1])):
            with pytest.raises(BigsiHipError) as e:
                call()
            assert e.value.code == ERR_STATE
    finally:
        b.delete()
