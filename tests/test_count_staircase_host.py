"""CPU side of tests/test_gpu_count_planes.py: for every case of tests/count_staircase.py the staircase is built and its CONDITIONS
are asserted on the numpy reference alone -- every target present exactly in each family, every named edge column at a target other
than 0, a column at min_kmers - 1, min_kmers and min_kmers + 1 of every threshold --, the reference is held against the C oracle on
the dense index, and the compiled launch planner (tests/c_host/launch_host.cpp) is asked which route the case's batch takes: a
planner change that moves a case off its route fails here instead of silently changing what the GPU test covers."""
import numpy as np
import pytest

from count_staircase import CASES, FAMILIES, K, build_case, min_kmers
from test_abi_and_host import build_launch_host, plan_on_host

NAMES = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_launch_host(tmp_path_factory.mktemp("launch_host"))


@pytest.mark.parametrize("name", NAMES)
def test_conditions_hold_on_the_reference(name):
    c, sc, queries = build_case(name)
    u, counts = sc.reference(sc.main)
    assert u == sc.u < c["main_pos"] == len(sc.main) - K + 1
    # every target, exactly, in each family -- and nothing else anywhere
    general = c.get("late_from") or c["n_cols"]
    for f in FAMILIES:
        assert sorted(t for col, t, fam in sc.columns if fam == f and col < general) == sc.targets, f
    assert {0, 1, u - 1, u} <= set(sc.targets)
    p = 0
    while (1 << p) <= u:
        assert (1 << p) - 1 in sc.targets and (1 << p) in sc.targets
        p += 1
    cols = np.array([col for col, _, _ in sc.columns])
    assert len(set(cols.tolist())) == cols.size
    assert np.array_equal(counts[cols], np.array([t for _, t, _ in sc.columns])), name
    rest = np.ones(c["n_cols"], bool)
    rest[cols] = False
    assert not counts[rest].any()
    # the edges
    wv = -(-c["n_cols"] // 64)
    assert {0, 63, 64, 127, c["n_cols"] - 1, 64 * (wv - 1)} <= set(sc.edges)
    if wv > 512:
        assert {64 * 511, 64 * 512 - 1, 64 * 512} <= set(sc.edges)          # the last word of the first 256-thread tile, the first of the second
    assert (counts[sc.edges] > 0).all(), name
    # the thresholds: min_kmers once a power of two, once all ones below a plane; a column on, below and above each
    assert len(sc.mks) == 2 and sc.mks[0] & (sc.mks[0] - 1) == 0 and sc.mks[1] & (sc.mks[1] + 1) == 0
    for thr, mk in zip(sc.thresholds, sc.mks):
        assert mk == min_kmers(u, thr) and 1 < mk < u
        for t in (mk - 1, mk, mk + 1):
            assert (counts == t).any(), (name, thr, t)
    if c.get("late_from"):
        # the columns of the second wavefront: late family, at min_kmers - 1 and min_kmers only
        late = counts[c["late_from"]:]
        assert set(late[late > 0].tolist()) == {t for mk in sc.mks for t in (mk - 1, mk)}
        assert all(f == "late" for col, _, f in sc.columns if col >= c["late_from"])
    # the batch: main first, fillers substrings of it, no longer than the main
    assert len(queries) == c["n_queries"] and queries[0] == sc.main
    assert all(q in sc.main for q in queries[1:])
    us = [sc.reference(q)[0] for q in queries[1:]]
    if len(us) >= 8:
        assert min(us) == 0 and any(0 < x < 10 for x in us) and any(10 <= x < 96 for x in us)
        assert len(queries[3]) < K
    if len(us) >= 64:
        assert {x % 8 for x in us} == set(range(8))
        assert sum(sc.reference(q)[1].any() for q in queries[1:65]) >= 32          # fillers get counts of their own from the same columns


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["main_pos"] <= 4096])
def test_reference_equals_the_c_oracle(name):
    from oracle import coracle
    c, sc, queries = build_case(name)
    dense = sc.dense()
    for q in [queries[0]] + queries[1:40:3]:
        u, counts = sc.reference(q)
        if len(q) < K:
            assert u == 0 and not counts.any()
            continue
        ou, ocounts, _ = coracle.query(dense, c["h"], q, K, want_and=False)
        assert ou == u and np.array_equal(ocounts[:c["n_cols"]].astype(np.int64), counts), (name, len(q))


@pytest.mark.parametrize("name", NAMES)
def test_case_takes_its_route(planner, name):
    c, sc, queries = build_case(name)
    wv = -(-c["n_cols"] // 64)
    max_pos = max(len(q) - K + 1 for q in queries)
    assert max_pos == c["main_pos"]
    if c["one_launch"]:
        # k_reads_fused takes the batch (reads_fusable, bigsi_hip.hip): reads of < 64 positions, rows of at most 512 words, h = 2 .. 4,
        # hits only.  Its three layouts: at most 64 reads on rows of at most 256 words split the workgroup; rows of at most 256 words
        # take one word per lane; wider ones two.
        assert c["route"] is None and max_pos <= 63 and wv <= 512 and c["h"] in (2, 3, 4) and c["sparse"] and not c["early"]
        kind = "split" if (wv <= 256 and c["n_queries"] <= 64) else "narrow" if wv <= 256 else "two"
        assert name.startswith("R" + kind)
        return
    head, ls = plan_on_host(planner, c["n_queries"], wv, max_pos, h=c["h"], exact=False, early_exit=c["early"], sparse_counts=c["sparse"])
    assert len(ls) == 1 and head["too_large"] == 0
    got = {k: head[k] for k in ("P", "count_bytes", "slices", "planes_out", "combine", "deep", "early")}
    got.update(block=ls[0]["block"], tiles=ls[0]["tiles"])
    assert got == c["route"], name
    assert ls[0]["slices"] == head["slices"] and (ls[0]["q0"], ls[0]["q1"]) == (0, c["n_queries"])
    # k_count_combine: all slices in one batch of loads when a slice leaves at most 4 planes (and there are at most 96), else its loop
    if head["combine"]:
        assert (head["planes_out"] <= 4) == (c["main_pos"] <= 1024) and head["slices"] <= 96
    if name == "Smix":
        # queries whose k-mers fill only some of the slices: live < slices
        assert any(0 < sc.reference(q)[0] < head["slices"] for q in queries[1:])
    # not a batch the read kernel would take instead
    assert not (max_pos <= 63 and c["sparse"])
