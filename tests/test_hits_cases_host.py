"""CPU side of tests/test_gpu_hit_lists.py: every case of tests/hits_cases.py is built, the compiled planner
(tests/c_host/hits_plan_host.cpp) is asked which path each of its calls takes through K4 and what the export carries along -- a
planner change that moves a case off its path fails here instead of silently changing what the GPU test covers -- and the numpy
reference is held to the edges the case names: the totals on the export's size and the lists' capacity, a hit on both sides of every
named cut, a group cut with a hit either side.  The reference itself is held against the C oracle on the dense index."""
import numpy as np
import pytest

import hits_cases as hc
from hits_cases import BLOCK, CAPACITY, K, WORD, build_case
from test_hits_plan_host import build_hits_host, plan, spec


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_hits_host(tmp_path_factory.mktemp("hits_cases_host"))


def hit_set(b, q):
    return set(b.reference()[q][3].tolist())


@pytest.mark.parametrize("name,mode", hc.PARAMS)
def test_case_takes_its_path(planner, name, mode):
    b = build_case(name, mode)
    c = b.case
    paths = b.paths()
    assert len(paths) == len(b.calls) >= 1
    cap = CAPACITY
    for call, p in zip(b.calls, paths):
        s = hc.shape_of(c, len(call))
        one_call = c["kind"] in ("one_call", "reads")
        cap = cap if one_call else CAPACITY
        assert p["capacity_before"] == cap
        if c["kind"] == "reads":
            # k_reads_fused takes the call (reads_fusable, bigsi_hip.hip): k = 31, at most 63 positions, rows of at most 512 words, h = 2 .. 4
            assert c["h"] in (2, 3, 4) and s["wv"] <= 512 and max(len(b.queries[q]) for q in call) - K + 1 <= 63
            assert sum(max(len(b.queries[q]) - K + 1, 0) for q in call) > 0
            assert (p["groups"], p["items_per_group"], p["single_workgroup"], p["one_launch"]) == (0, 0, 0, 1)
            assert p["inline_export"] == int(len(call) == 1)
        else:
            assert c["h"] == 1          # never the read kernel, whatever the lengths
            assert (p["items_per_group"], p["groups"], bool(p["single_workgroup"])) == plan(planner, s["items"], s["shards"])
            assert p["inline_export"] == int(one_call and p["single_workgroup"]) and p["one_launch"] == 0
            # the kernel's own test for its single-workgroup body
            assert bool(p["single_workgroup"]) == (p["groups"] == 1 and s["shards"] == 1 and s["chunks"] <= 16)
        assert p["exp_spec"] == (spec(planner, len(call), cap) if one_call else 0)
        assert p["rewrites"] == int(p["total"] > cap)
        assert p["collect_fetch"] == int(one_call and (p["total"] > cap or (c["kind"] == "reads" and p["total"] > p["exp_spec"])))
        cap = max(cap, p["total"])
    # what the table says about the case
    first = paths[0]
    want = {"one_100": (1, 1, 1), "one_16384": (1, 1, 1), "one_16385": (2, 1, 1), "one_70016": (5, 1, 1), "one_262144": (16, 1, 1),
            "one_262145": (1, 17, 0), "totals_first": (5, 1, 1), "totals_scattered": (5, 1, 1), "two_16": (16, 1, 1), "two_18": (1, 18, 0),
            "seventeen": (1, 17, 0), "b1024": (1, 1024, 0), "b1025": (2, 513, 0), "b700x3": (3, 700, 0), "b400x3": (2, 600, 0),
            "b_last_only": (1, 300, 0), "b_first_only": (1, 300, 0), "b_sparse": (2, 513, 0), "b_regrow": (1, 600, 0),
            "g2": (6, 1, 0), "g20": (1, 60, 0), "g400": (2, 600, 0)}
    if name in want:
        assert (first["items_per_group"], first["groups"], first["single_workgroup"]) == want[name]
        assert all((p["items_per_group"], p["groups"], p["single_workgroup"]) == want[name] for p in paths)
    if name == "b1025":
        assert 1025 - (first["groups"] - 1) * first["items_per_group"] == 1          # a last group of one
    if name in ("b1024", "b1025", "b_sparse", "seventeen", "b_last_only", "b_first_only", "g2", "g20", "g400", "r257", "r16400", "r_spec"):
        assert not any(p["rewrites"] or p["collect_fetch"] for p in paths)
    if name == "r16400":
        # k_export_reads: 64 workgroups of 257 queries, so that its loop over 256 queries runs twice -- and the query of the second
        # pass has hits in some workgroup
        rgrid = min(-(-16400 // BLOCK), 64)
        per_g = -(-16400 // rgrid)
        assert (rgrid, per_g) == (64, 257) and first["exp_spec"] == CAPACITY >= first["total"]
        assert sum(b.reference()[g * per_g + 256][3].size > 0 for g in range(rgrid - 1)) >= 20
    if name == "r257":
        assert min(-(-257 // BLOCK), 64) == 2 and first["exp_spec"] == 4112
    if name == "r300_all":
        assert first["exp_spec"] == 4800 < first["total"] == 300 * 128 <= CAPACITY and first["collect_fetch"] and not first["rewrites"]
    if name == "r_spec":
        assert first["total"] == first["exp_spec"] == 1040
    if name == "r_spec1":
        assert first["total"] == first["exp_spec"] + 1 == 1041 and first["collect_fetch"] and not first["rewrites"]


@pytest.mark.parametrize("name,mode", hc.PARAMS)
def test_reference_has_the_edges_the_case_names(name, mode):
    b = build_case(name, mode)
    c, ref, n = b.case, b.reference(), b.case["n_cols"]
    # the construction: distinct rows throughout, every query with as many unique k-mers as its mode wants, min_kmers 1 below 1.0
    from oracle import coracle
    rows = np.concatenate([coracle.seq_rows(q, K, c["h"], b.m).ravel() for q in b.queries])
    assert np.unique(rows).size == rows.size == b.row_ids.size and np.array_equal(np.sort(rows), b.row_ids)
    for what, (nk, u, mk, col, cnt) in zip(b.patterns, ref):
        assert nk == u == (0 if what == "short" else 1 if mode == "exact" else 2)
        assert mk == (u if mode == "exact" else min(u, 1))
        cols = hc.pattern_columns(c, what, np.random.default_rng(0)) if what not in ("half",) and not (isinstance(what, tuple) and what[0] == "scatter_n") else None
        if what == "short":
            assert col.size == (0 if mode == "exact" else n) and not cnt.any()
        else:
            if cols is not None:
                assert np.array_equal(col, cols), what
            assert np.array_equal(cnt, np.full(col.size, 1) if mode == "exact" else np.where(col % 3 == 0, 2, 1)), what
        assert np.all(np.diff(col.astype(np.int64)) > 0) and (col.size == 0 or col[-1] < n)
    if mode == "thr":
        seen = np.concatenate([r[4] for r in ref])
        assert {1, 2} <= set(np.unique(seen).tolist())
    # the menu: empty, every column, the first and the last column alone, one hit per word
    by_pattern = {what: q for q, what in reversed(list(enumerate(b.patterns))) if isinstance(what, str)}
    wv = -(-n // WORD)
    if "all" in by_pattern:
        assert ref[by_pattern["all"]][3].size == n
    if "first" in by_pattern and "last" in by_pattern:
        assert ref[by_pattern["first"]][3].tolist() == [0] and ref[by_pattern["last"]][3].tolist() == [n - 1]
    if "word" in by_pattern:
        assert np.array_equal(np.unique(ref[by_pattern["word"]][3] // WORD), np.arange(wv)) and ref[by_pattern["word"]][3].size == wv
    if "empty" in by_pattern:
        assert ref[by_pattern["empty"]][3].size == 0
    # every named cut: the last column of the word before it and the first column of the word behind it, in ONE query's list
    cuts = hc.word_cuts(c)
    named = sorted({w for ws in cuts.values() for w in ws})
    if "cuts" in b.patterns and named:
        got = hit_set(b, b.patterns.index("cuts"))
        for w in named:
            assert {WORD * w - 1, WORD * w} <= got, w
    s = hc.shape_of(c, len(b.calls[0]))
    if s["single"] and c["kind"] == "one_call":
        # thread t of the single-workgroup body owns the words chunks x t .. chunks x t + chunks - 1: a cut in front of every thread that owns any
        assert cuts["thread"] == [w for w in range(1, wv) if w % s["chunks"] == 0] and len(cuts["thread"]) == -(-wv // s["chunks"]) - 1
    if s["chunks"] > 1 and c["kind"] != "group":
        assert cuts["chunk"] == [BLOCK * i for i in range(1, s["chunks"])]
    # totals on the export's size and on the capacity
    totals = [p["total"] for p in b.paths()]
    if name.startswith("totals_"):
        assert totals[:6] == [1023, 1024, 1025, 65535, 65536, 65537] and 0 < totals[6] < 1024 and totals[7] == 1
        assert [p["exp_spec"] for p in b.paths()] == [1024] * 8 and [p["capacity_before"] for p in b.paths()] == [CAPACITY] * 6 + [65537] * 2
        assert [p["collect_fetch"] for p in b.paths()] == [0, 0, 0, 0, 0, 1, 0, 0]
        if name == "totals_scattered":
            for q in range(6):
                col = ref[q][3]
                assert col[0] == 0 and col[-1] == n - 1 and np.unique(col // (WORD * BLOCK)).size == s["chunks"]
    if name == "one_262145":
        assert totals[-3:] == [1023, 1024, 1025]
    if name == "b_last_only":
        assert [r[3].size for r in ref[:-1]] == [0] * 299 and ref[-1][3].size == n and s["groups"] > 256
    if name == "b_first_only":
        assert [r[3].size for r in ref[1:]] == [0] * 299 and ref[0][3].size == n and s["groups"] > 256
    if name == "b_regrow":
        running = np.cumsum([r[3].size for r in ref])
        q = int(np.searchsorted(running, CAPACITY, side="right"))          # the query in whose list entry 65 536 lies
        assert q == 400 and running[q - 1] < CAPACITY < running[q] and s["groups"] // 4 < q * s["chunks"] // s["ipb"] < 3 * s["groups"] // 4
        assert running[-1] > running[q] and b.paths()[0]["rewrites"] == 1
    # group cuts of the general body: an item boundary at a multiple of ipb with a hit in the last valid column of the item before it
    # and in the first column of the item behind it -- inside a vector (a chunk cut) and, where groups end on vectors, across two
    if not s["single"] and c["kind"] in ("batch", "group", "one_call") and s["groups"] > 1:
        inside = across = 0
        for call, g in ((call, g) for call in b.calls for g in range(1, s["groups"])):
            i = g * s["ipb"]
            sides = []
            for item, last in ((i - 1, True), (i, False)):
                chunk, sq = item % s["chunks"], item // s["chunks"]
                shard, q = sq % s["shards"], sq // s["shards"]
                lo = shard * s["width"] + chunk * BLOCK * WORD
                hi = min(shard * s["width"] + min((chunk + 1) * BLOCK * WORD, s["width"]), n)
                sides.append((q, shard, (hi - 1) if last else lo, hi > lo))
            (q0, sh0, c0, ok0), (q1, sh1, c1, ok1) = sides
            if ok0 and ok1 and c0 in hit_set(b, call[q0]) and c1 in hit_set(b, call[q1]):
                inside += (q0, sh0) == (q1, sh1)
                across += (q0, sh0) != (q1, sh1)
        if s["chunks"] > 1 and s["ipb"] % s["chunks"]:
            assert inside >= 1, "no group cut inside a vector has a hit on both sides"
        if len(b.calls[0]) * s["shards"] > 1 and (s["ipb"] == 1 or s["chunks"] == 1 or s["ipb"] % s["chunks"] == 0 or s["chunks"] % s["ipb"]):
            assert across >= 1 or name in ("b_last_only", "b_first_only"), "no group cut between two vectors has a hit on both sides"
    if c["kind"] == "group":
        sc = c["shard_cols"]
        assert (sc, [min(sc, max(n - i * sc, 0)) for i in range(3)]) == (384, [384, 384, 232])          # uneven shards
        sides = [q for q in range(len(ref)) if {sc - 1, sc} <= hit_set(b, q) and {2 * sc - 1, 2 * sc} <= hit_set(b, q)]
        assert sides, "no query with hits on the last column of a shard and the first of the next"
        skipping = [q for q in range(len(ref)) if 0 < ref[q][3].size < n and {int(x) // sc for x in ref[q][3]} == {0, 2}]
        assert skipping, "no query whose middle shard is without hits"
        if name != "g2":
            assert any({int(x) // sc for x in r[3]} == {1} for r in ref if r[3].size)


@pytest.mark.parametrize("name,mode", [(n, m) for n, m in hc.PARAMS if n in ("one_100", "one_16385", "r257", "r_spec1", "g20", "seventeen")])
def test_reference_equals_the_c_oracle(name, mode):
    from oracle import coracle
    b = build_case(name, mode)
    c = b.case
    dense = np.zeros((b.m, b.packed.shape[1]), np.uint8)
    dense[b.row_ids.astype(np.int64)] = b.packed
    for q, seq in list(enumerate(b.queries))[:40]:
        nk, u, counts = b.counts(seq)
        if len(seq) < K:
            assert (nk, u) == (0, 0) and not counts.any()
            continue
        ou, ocounts, _ = coracle.query(dense, c["h"], seq, K, want_and=False)
        assert ou == u and np.array_equal(ocounts[:c["n_cols"]].astype(np.int64), counts), (name, q)
