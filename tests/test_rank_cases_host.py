"""CPU side of tests/test_gpu_rank_select.py: the numpy reference of the top-N selection (tests/rank_cases.py) is held against a
brute-force sorted() and against the ordering model that is pinned to the reference's own results (model_top_n,
tests/test_search_limit_host.py); every direct case is shown to reach the branch it is named for -- analyse() walks the kernel's steps
over the case's arrays (digit passes, the cutoff bin of each, what still fits, the tile, thread and bit of the cut, the ties carried
from earlier tiles) and the case's declared edge must equal that; the case groups are shown to hold every edge the kernel has; and
every staircase case is built, its conditions asserted on the numpy reference alone, and the compiled planner
(tests/c_host/launch_host.cpp) asked for the route of its batch."""
import numpy as np
import pytest

import rank_cases as rc
from count_staircase import K, min_kmers
from test_abi_and_host import build_launch_host, plan_on_host
from test_search_limit_host import model_top_n


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_launch_host(tmp_path_factory.mktemp("launch_host"))


def test_row_format_round_trip():
    rng = np.random.default_rng(0)
    bits = rng.random(64 * 5) < 0.4
    words = rc.pack_cols(bits)
    assert np.array_equal(rc.unpack_words(words), bits)
    # column 8b + j of a word sits at bit 8b + 7 - j (bit_of_col, bigsi_kernels.hpp)
    for col in (0, 7, 8, 63, 64, 100, 319):
        assert rc.words_of([col], 5)[col // 64] == np.uint64(1) << np.uint64(8 * (col % 64 // 8) + 7 - col % 8)
    assert not rc.words_of([320, 10 ** 6], 5).any()


def random_query(rng, wv, stride, exact):
    bits = rng.random(64 * stride) < rng.choice([0.05, 0.5])
    mk = int(rng.integers(0, 20))
    nu = mk + int(rng.choice([0, 2, 5, 5000]))
    counts = None if exact else rng.integers(mk, nu + 1, size=64 * stride)          # few values: ties at every cut
    excluded = rng.integers(0, 64 * stride + 50, size=int(rng.integers(0, 12))).tolist()
    return rc.pack_cols(bits), counts, nu, mk, excluded


def test_reference_equals_brute_force_and_the_ordering_model():
    rng = np.random.default_rng(11)
    checked = cut_in_ties = 0
    for it in range(300):
        wv = int(rng.integers(1, 6))
        stride = wv + int(rng.integers(0, 3))
        exact = bool(it % 3 == 0)
        words, counts, nu, mk, excluded = random_query(rng, wv, stride, exact)
        preset = rng.integers(0, 1 << 63, size=stride).astype(np.uint64)
        hit = [c for c in range(64 * wv) if rc.unpack_words(words)[c]]
        for limit in (1, 2, 7, 40, 10 ** 6):
            got = rc.reference(words, counts, nu, mk, excluded, limit, wv=wv, preset=preset)
            assert np.array_equal(got[wv:], preset[wv:])
            assert np.array_equal(rc.reference(words, counts, nu, mk, excluded, limit, wv=wv)[wv:], words[wv:])
            kept = np.flatnonzero(rc.unpack_words(got[:wv])).tolist()
            # brute force: plain Python over (count, colour) pairs
            left = [c for c in hit if c not in set(excluded)]
            brute = left if len(left) <= limit else sorted(left)[:limit] if exact else sorted(left, key=lambda c: (-int(counts[c]), c))[:limit]
            assert kept == sorted(brute), (it, limit)
            # the model pinned to the reference's own result lists
            model = model_top_n(hit[::-1], [nu if exact else int(counts[c]) for c in hit[::-1]], limit, exact, excluded)
            assert kept == sorted(model), (it, limit)
            if not exact and len(left) > limit:
                order = sorted(left, key=lambda c: (-int(counts[c]), c))
                cut_in_ties += counts[order[limit - 1]] == counts[order[limit]]
            checked += 1
    assert checked == 1500 and cut_in_ties >= 100


@pytest.mark.parametrize("name", [c["name"] for c in rc.DIRECT])
def test_direct_case_reaches_its_edge(name):
    c = next(x for x in rc.DIRECT if x["name"] == name)
    got = rc.analyse(c)
    assert c["edge"], "a case declares what it is for"
    for key, want in c["edge"].items():
        if key == "base_min":
            assert got["base"] >= want, (name, key, got["base"])
        else:
            assert got.get(key) == want, (name, key, got.get(key), want)
    # the arrays are what the kernel may be given: hits inside wv, counts of hits inside [min_kmers, num_unique], junk elsewhere
    assert c["cols"].size == 0 or c["cols"][-1] < 64 * c["wv"] - rc.RAGGED
    if c["counts"] is not None:
        junk = rc.JUNK32 if c["cbytes"] == 4 else rc.JUNK16
        mask = np.zeros(c["counts"].size, bool)
        mask[c["cols"]] = True
        assert (c["counts"][~mask] == junk).all()
        assert ((c["counts"][mask] >= c["mk"]) & (c["counts"][mask] <= c["nu"])).all()
    # and the reference agrees with the analysis: the kept ties end at the cut, the first dropped one is out
    words = rc.words_of(c["cols"], c["wv"])
    kept = np.flatnonzero(rc.unpack_words(rc.reference(words, c["counts"], c["nu"], c["mk"], c["excluded"], c["limit"])))
    assert kept.size == min(c["limit"], got["total"])
    if not got["early"]:
        col = lambda t: (t[0] * rc.TILE + t[1]) * 64 + t[2]          # noqa: E731
        assert col(got["cut"]) in kept and (got["drop"] is None or col(got["drop"]) not in kept)


def test_direct_groups_hold_every_edge():
    A = {c["name"]: (c, rc.analyse(c)) for c in rc.DIRECT}
    by = lambda g: [(c, a) for c, a in A.values() if c["group"] == g]          # noqa: E731
    live = lambda g: [(c, a) for c, a in by(g) if not a["early"]]              # noqa: E731
    # early return: total = limit - 1, limit, limit + 1 and 0, with and without excluded words, and the exclusion alone reaching the limit
    for exact in (True, False):
        e = [(c, a) for c, a in by("early") if (c["counts"] is None) == exact]
        for ex in (False, True):
            assert {a["total"] - c["limit"] for c, a in e if bool(c["excluded"]) == ex} >= {-1, 0, 1}
            assert any(a["total"] == 0 for c, a in e if bool(c["excluded"]) == ex)
        assert any(a["early"] and len(c["cols"]) > c["limit"] >= a["total"] for c, a in e)
    # exact runs: every width, last word ragged, and the cuts
    x = live("exact")
    assert {c["wv"] for c, _ in x} == {1, 2, 255, 256, 257, 513, 600}
    cuts = {(c["wv"], a["cut"], a["drop"]) for c, a in x}
    assert any(cut[2] == 0 for _, cut, _ in cuts) and any(cut[2] == 63 and drop[2] == 0 for _, cut, drop in cuts)              # first / last bit of a word
    assert any(cut[:2] == drop[:2] and cut[2] // 8 == drop[2] // 8 and 0 < drop[2] % 8 for _, cut, drop in cuts)             # the middle of a byte
    assert any(cut[1] == 63 and drop[1] == 64 and cut[0] == drop[0] for _, cut, drop in cuts)                               # lane 63 | 64
    assert any(cut[:2] == (0, 255) and drop[:2] == (1, 0) for _, cut, drop in cuts)                                         # word 255 | 256
    assert any(cut[:2] == (1, 255) and drop[:2] == (2, 0) for _, cut, drop in cuts)                                         # word 511 | 512
    assert all(any(w == wv and (cut[0] * 256 + cut[1] == wv - 1) for w, cut, _ in cuts) for wv in (1, 255, 257, 600))        # inside the ragged last word
    assert sum(c["limit"] == 1 and a["base"] == 0 and a["cut"][0] == a["tiles"] - 1 > 0 and c["cols"][0] // 64 // 256 == a["tiles"] - 1 for c, a in x) >= 3
    assert any(a["base"] > 0 and a["cut"][0] == 2 for _, a in x)
    # one digit
    d1 = live("one digit")
    assert all(a["passes"] == 1 for _, a in d1)
    assert any(a["bins"] == [0] and a["n_ties"] == a["total"] for _, a in d1)                                                  # all counts at mk
    assert any(a["bins"] == [4095] and a["n_ties"] == a["total"] and c["nu"] - c["mk"] == 4095 for c, a in d1)                 # all at num_unique, range 4095
    for b in (0, 15, 16, 1023, 1024, 4095):
        rems = {(a["remaining"], a["hist"]) for _, a in d1 if a["bins"] == [b]}
        assert (1, 4) in rems and (2, 4) in rems and (b == 0 or (4, 4) in rems), b
    # two digits
    d2 = live("two digits")
    assert all(a["passes"] == 2 for _, a in d2)
    assert {a["cutoff"] - c["mk"] for c, a in d2 if c["nu"] - c["mk"] == 4096} >= {4096, 4095, 0}
    assert {a["cutoff"] - c["mk"] for c, a in d2 if c["nu"] - c["mk"] == 8192} >= {4095, 4096, 4097, 8191, 8192}
    assert {a["cutoff"] for c, a in d2 if c["cbytes"] == 2} >= {65535} and {a["cutoff"] for c, a in d2 if c["cbytes"] == 4} >= {65536, 65537}
    assert any(a["remaining"] == a["hist"] for _, a in d2) and any(a["remaining"] == 1 < a["hist"] for _, a in d2)
    # three digits
    d3 = live("three digits")
    T = 1 << 24
    assert {a["passes"] for c, a in d3 if c["nu"] - c["mk"] == T - 1} == {2} and {a["passes"] for c, a in d3 if c["nu"] - c["mk"] >= T} == {3}
    assert {a["cutoff"] - c["mk"] for c, a in d3 if a["passes"] == 3} >= {T - 1, T, T + 1}
    assert all(c["cbytes"] == 4 for c, _ in d3)
    firsts = {a["bins"][0] for _, a in d3 if a["passes"] == 3}
    assert {0, 1} <= firsts
    # tie geometry
    t = live("tie geometry")
    assert any(a["base"] > 0 and a["cut"][0] == 2 and c["counts"] is not None for c, a in t)
    tiles_of = lambda c, a: {int(x) // 64 // 256 for x in c["cols"][np.maximum(c["counts"][c["cols"]] - c["mk"], 0) == a["cutoff"] - c["mk"]]}          # noqa: E731
    assert any(tiles_of(c, a) == {0, 2} for c, a in t)                                                                          # none in tile 1
    assert any(a["cut"][:2] == (0, 255) and a["drop"][:2] == (2, 0) for _, a in t)
    assert any(a["cut"][1] == 63 and a["drop"][1] == 64 for _, a in t)
    # excluded colours
    xc = by("excluded colours")
    ex = set().union(*[set(c["excluded"]) for c, _ in xc])
    assert {0, 63, 64} <= ex and any(e == 64 * c["wv"] - rc.RAGGED - 1 for c, _ in xc for e in c["excluded"])
    assert any(e >= 64 * c["wv"] for c, _ in xc for e in c["excluded"])
    assert any(set(c["cols"][c["cols"] // 64 == 1].tolist()) <= set(c["excluded"]) and (c["cols"] // 64 == 1).any() for c, _ in xc)
    # every direct case runs with others of its call where the tables allow it, and none is alone in the table of its group
    assert len(rc.DIRECT) >= 120


def test_fuzz_call_is_seeded_and_well_formed():
    a, b = rc.fuzz_call(5, n_seqs=8, wv=40), rc.fuzz_call(5, n_seqs=8, wv=40)
    assert np.array_equal(a["hits"], b["hits"]) and np.array_equal(a["counts"], b["counts"]) and a["limit"] == b["limit"]
    assert a["hits"].shape == (8, 43) and a["counts"].shape == (8, 64 * 43)
    for q in range(8):
        hit = rc.unpack_words(a["hits"][q][:40])
        c = a["counts"][q][:64 * 40]
        assert ((c[hit] >= a["mk"][q]) & (c[hit] <= a["nu"][q])).all() and (c[~hit] == rc.JUNK16).all()
    assert rc.fuzz_call(6, n_seqs=4, wv=10, cbytes=0)["counts"] is None


def test_entry_point_refuses_bad_arguments_without_a_device():
    """bigsi_hip_rank_select_arrays: NULL arrays, wv beyond the stride, a counter width other than 2 or 4, counters without
    num_unique / min_kmers and limit == 0 are BIGSI_ERR_INVALID before any device work -- here there is no device to do any on."""
    from bigsi_amd import _lib
    L = _lib.lib()
    hits, out = np.zeros((2, 4), np.uint64), np.full((2, 4), rc.PRESET, np.uint64)
    cnt, nu = np.zeros((2, 256), np.uint16), np.zeros(2, np.uint32)
    good = [0, _lib.ptr(hits), 4, 3, 2, _lib.ptr(cnt), 2, _lib.ptr(nu), _lib.ptr(nu), None, 5, 0, _lib.ptr(out)]
    for i, bad in ((1, None), (12, None), (3, 5), (6, 3), (6, 8), (6, 0), (10, 0), (7, None), (8, None)):
        args = list(good)
        args[i] = bad
        assert L.bigsi_hip_rank_select_arrays(*args) == _lib.ERR_INVALID, (i, bad)
        assert L.bigsi_hip_last_error()
    assert (out == rc.PRESET).all()


# --------------------------------------------------------------------------------------------- layer E
@pytest.mark.parametrize("name", [c["name"] for c in rc.STAIR_CASES])
def test_staircase_case_conditions_and_route(planner, name):
    c, sc, queries, thr, tie = rc.build_stair(name)
    u, counts = sc.reference(sc.main)
    mk = min_kmers(u, thr)
    assert u == sc.u and mk == c["mk_of"](u) and queries[0] == sc.main and len(queries) == c["n_queries"]
    # every column at its target, nothing else anywhere
    cols = np.array([col for col, _, _ in sc.columns])
    assert np.array_equal(counts[cols], [t for _, t, _ in sc.columns])
    rest = np.ones(c["n_cols"], bool)
    rest[cols] = False
    assert not counts[rest].any()
    # the tie block: one (target, family) across 61 .. 66, 16 380 .. 16 390 on the wide index, and the last columns of the ragged word
    block = rc.tie_block(c["n_cols"])
    # (the wide index is 513 full words; its ragged words are the shards' of the group case: 16 416 columns are 256.5 words)
    assert (c["n_cols"] % 64 or c["n_cols"] == 2 * 16416) and set(range(61, 67)) <= set(block) and set(range(c["n_cols"] - 4, c["n_cols"])) <= set(block)
    assert (c["n_cols"] > 16390) == (set(range(16380, 16391)) <= set(block))
    assert (counts[block] == tie).all() and np.flatnonzero(counts == tie).tolist() == sorted(block)
    assert {f for col, _, f in sc.columns if col in block} == {"early"}
    hit = counts >= mk
    higher = np.flatnonzero(hit & (counts > tie))
    assert higher.size >= 6 and higher[0] < block[0] and higher[-1] > block[-5] and ((higher > 66) & (higher < c["n_cols"] - 4)).any()
    assert (hit & (counts < tie)).any() and (mk == 0 or (counts[cols] == mk - 1).any())
    # the limits put the cut at 63 | 64, inside bytes, at 16 383 | 16 384 on the wide index and inside the ragged word; T - 1, T, T + 1 run too
    lims = rc.stair_limits(sc, tie, counts, mk, exact=c["exact"])
    T = int((counts == u).sum()) if c["exact"] else int(hit.sum())
    assert {T - 1, T, T + 1} <= set(lims)
    if not c["exact"]:
        order = rc.ranked_order(np.flatnonzero(hit), counts[hit])
        last_kept = {int(order[n - 1]) for n in lims if n <= T}
        assert {61, 63, 66, c["n_cols"] - 2} <= last_kept and (c["n_cols"] < 16390 or {16383, 16384, 16390} <= last_kept)
    # two digits / 32-bit: the counts the case is named for are there
    if name == "E_two_digits":
        assert u == 65530 and mk == 0 and hit.all() and {4095, 4096, 4097, 8191, 8192, u - 1, u} <= set(counts.tolist())
    if name == "E_32bit":
        assert u > 65537 and {65535, 65536, 65537, mk + 4095, mk + 4096} <= set(counts.tolist())
    # the route
    wv = -(-c["n_cols"] // 64)
    max_pos = max(len(q) - K + 1 for q in queries)
    assert max_pos == c["main_pos"]
    if c["devices"]:
        assert c["n_cols"] == 2 * 16416 and -(-16416 // 64) == 257          # two shards of 257 words: each member trims more than one tile in place
        wv = 257
    head, ls = plan_on_host(planner, c["n_queries"], wv, max_pos, h=c["h"], exact=c["exact"], sparse_counts=c["sparse"] or bool(c["devices"]))
    assert head["too_large"] == 0
    if c["route"] is not None:
        got = {k: head[k] for k in ("P", "count_bytes", "slices", "planes_out", "combine", "deep", "early")}
        got.update(block=ls[0]["block"], tiles=ls[0]["tiles"])
        assert len(ls) == 1 and got == c["route"], (name, got)
    assert wv > 256 or not name.startswith(("E_wide", "E_group"))
    assert not (max_pos <= 63 and c["sparse"])          # (not a batch the read kernel would take)
