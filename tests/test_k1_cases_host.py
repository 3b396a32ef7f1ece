"""CPU-only: the cases of the K1 edge tests (tests/k1_cases.py) held to what they promise before the device sees them.
(1) The plain-Python reference against the recorded reference-project data (tests/golden/g1_hash.json: raw mmh3 values,
generate_hashes, canonical, reverse_comp) and, for every case, against the C oracle (seq_rows, unique_kmers).  (2) Coverage, computed
from the reference and the planner exports alone: every (route, first-difference byte, outcome, alignment) combination, the ties, the
homopolymer sizes, the straddling repeats, the fingerprint collisions, the wrapping probe chains, the isolation layout, the
run-time k shapes and the modulus branches are in the table -- the condition that keeps the GPU test from thinning out silently.
(3) Every run of every case takes the instance it is built for: the restated launch rule of k1_cases.expected_route against the
compiled planner (tests/c_host/launch_host.cpp).  (4) The planted-index searches on the CPU twin (libbigsi_cpu.so): a third
implementation pinned to the same reference.  (5) Sensitivity: a Python restatement of kmer31_canonical_premix's eight-word
big-endian compare agrees with the reference on every placement, and with the decision of word 0, 1, 2 or 3 inverted it disagrees
on set A at every alignment (the side a tie takes cannot be observed); the same for the select chain of
RegKmer<31>::canonical_words with one step the wrong way round or the chain cut short."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import k1_cases as kc
from conftest import ROOT, load_golden
from k1_cases import CASES, K, SHAPES, SHAPE_OF, ceil_thr, first_difference, ref_of
from oracle import coracle
from raw_index import ptr

NAMES = [c["name"] for c in CASES]
CPU_LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("k1_host") / "liblaunch_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "c_host", "launch_host.cpp")])
    L = C.CDLL(so)
    L.launch_host_plan.restype = C.c_uint64
    L.launch_host_sort_rows_block.restype = C.c_uint32
    L.launch_host_sort_rows_block.argtypes = [C.c_uint64, C.c_uint32]
    return L


def planner_k1(L, n_seqs, max_pos, max_len, force_global):
    out = np.zeros(6, np.uint64)
    L.launch_host_k1_plan(C.c_uint32(n_seqs), C.c_uint64(max_pos), C.c_uint64(max_len), 0, int(force_global), ptr(out))
    return dict(zip(("route", "hs_cap", "sq_bytes", "tab_mult", "tab_cap", "lds"), out.tolist()))


def planner_want_sorted(L, n_seqs, wv, max_pos, h, exact):
    head, launches = np.zeros(11, np.uint64), np.zeros(8 * 64, np.uint64)
    L.launch_host_plan(C.c_uint32(n_seqs), C.c_uint64(wv), C.c_uint64(max_pos), C.c_uint32(h), int(exact), 0, 0, 0, ptr(head), ptr(launches), C.c_uint64(64))
    return int(head[2])


def runs_of(c):
    """[(threshold, run_kw, built_for, expected route)] of a case"""
    assert len(c["built_for"]) == len(c["runs"])
    return [(thr, kw, bf, kc.expected_route(c["queries"], c["k"], c["h"], c["n_cols"], thr, kw)) for (thr, kw), bf in zip(c["runs"], c["built_for"])]


def instances_of(c):
    return {(e["instance"], e["k1_parts"]) for _, _, _, e in runs_of(c)}


# --------------------------------------------------------------------------------------------- (1) the reference
def test_reference_equals_the_recorded_reference_project_data():
    g = load_golden("g1_hash.json")
    signed = lambda v: v - (1 << 32) if v >= 1 << 31 else v      # noqa: E731
    for rec in g["mmh3"]:
        assert [signed(kc.murmur3_32(rec["s"].encode("utf-8"), seed)) for seed in g["seeds"]] == rec["hashes"], rec["s"]
    for rec in g["generate_hashes"]:
        rows = [signed(kc.murmur3_32(rec["s"].encode("utf-8"), seed)) % rec["m"] for seed in range(rec["h"])]
        assert rows == rec["rows_in_seed_order"] and sorted(set(rows)) == rec["set"], rec
    for rec in g["canonical"]:
        assert kc.revcomp(rec["s"]) == rec["reverse_comp"] and kc.canonical(rec["s"]) == rec["canonical"], rec
    for rec in g["seq_to_kmers"]:
        r = kc.Ref(rec["seq"], rec["k"])
        assert [rec["seq"][p:p + rec["k"]] for p in range(r.n)] == rec["kmers"] and sorted(r.uniq) == sorted(set(rec["kmers"]))
    assert [ceil_thr(u, t) for u, t in ((0, 1.0), (7, 0.5), (7, 0.0), (10, 0.3), (3, 1.0))] == [0, 4, 0, 3, 3]
    # (k1_cases restates count_staircase.min_kmers so that it imports nothing of the project: the two are one function)
    import count_staircase
    assert all(ceil_thr(u, t) == count_staircase.min_kmers(u, t) for u in range(0, 4200, 7) for t in (1.0, 0.5, 0.0, 0.3, 0.7, -0.1, 1 / 3))


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_oracle_on_every_case(name):
    c = kc.CASE_BY_NAME[name]
    k, h, m = c["k"], c["h"], c["m"]
    for q in dict.fromkeys(c["queries"]):
        r = ref_of(q, k)
        first, p2u = coracle.unique_kmers(q, k)
        assert first.tolist() == r.first and p2u.tolist() == r.pos_unique, (name, q[:40])
        assert r.rep == [r.first[t] for t in r.pos_unique] and r.uniq == [q[p:p + k] for p in r.first]
        if r.u:
            assert coracle.seq_rows(q, k, h, m)[first].tolist() == r.rows(h, m), (name, q[:40])
        if r.u and r.u <= 8:
            assert [coracle.kmer_rows(km, h, m) for km in r.uniq] == r.rows(h, m)


def test_shapes_are_what_they_are_named():
    assert [key for key, _ in SHAPES] == [(j, who) for j in range(16) for who in ("fwd", "rc")] + [(None, "tie")]
    for (j, who), s in SHAPES:
        assert len(s) == K and first_difference(s) == (j, who)
        assert coracle.canonical(s) == kc.canonical(s) == (coracle.reverse_comp(s) if who == "rc" else s)
        assert who != "tie" or (s[15] == "N" and kc.revcomp(s) == s)
    # the first difference of ANY 31-mer lies at byte 15 at the latest: differences come in mirrored pairs
    rng = np.random.default_rng(1)
    for _ in range(2000):
        s = "".join(rng.choice(list("ACGTNacgt"), size=K))
        j, _ = first_difference(s)
        assert j is None or j <= 15


# --------------------------------------------------------------------------------------------- (2) coverage
def test_reads_batch_holds_every_placement_under_every_rotation():
    q = kc.CASE_BY_NAME["reads"]["queries"]
    assert len(q) == 1024 and max(len(s) for s in q) <= 93
    for blk in range(4):
        body = q[256 * blk:256 * blk + 66]
        assert kc.placements_in(body) >= kc.ALL_PLACEMENTS, blk
        # every shape at the first position of a sequence and at the last position of one
        assert {s[:K] for s in body} >= set(SHAPE_OF.values()) and {s[-K:] for s in body} >= set(SHAPE_OF.values())
        assert all(len(s) == K for s in q[256 * blk + 100:256 * (blk + 1)])          # (the rest: 31-byte queries)
    # the same batch five ways, and on an index of one hash
    assert [bf for _, _, bf, _ in runs_of(kc.CASE_BY_NAME["reads"])] == ["k_reads_fused", "k_reads_fused", "k_kmerize_wave<31>", "k_kmerize_wave<31>", "k_kmer_rows<31>"]
    assert kc.CASE_BY_NAME["reads_h1"]["queries"] is q and kc.CASE_BY_NAME["reads_h1"]["h"] == 1
    # lane 63 of the wave route: queries of exactly 64 positions whose last k-mer is a late-deciding shape
    w = [s for s in kc.CASE_BY_NAME["wave64"]["queries"] if len(s) == 94]
    assert {first_difference(s[63:]) for s in w} >= {(15, "fwd"), (15, "rc"), (None, "tie"), (8, "rc")}


def test_lds_cases_hold_every_placement_and_every_part_a_deep_shape():
    shape_q = [s for s in kc.CASE_BY_NAME["lds_shapes"]["queries"] if len(s) >= 95]
    assert kc.placements_in(shape_q) >= kc.ALL_PLACEMENTS and all(65 <= len(s) - K + 1 <= 200 for s in shape_q)
    assert kc.placements_in(kc.CASE_BY_NAME["lds_sorted"]["queries"]) >= kc.ALL_PLACEMENTS
    assert {e["sorted_by"] for _, _, _, e in runs_of(kc.CASE_BY_NAME["lds_sorted"])} == {kc.BY_K1, kc.NONE}
    # parts = 8: the share of part i is the unique k-mers [i * per_j, (i + 1) * per_j), per_j = ceil(u / 8)
    c = kc.CASE_BY_NAME["lds_parts8"]
    assert all(e["k1_parts"] == 8 and e["k1_route"] == kc.K1_LDS for _, _, _, e in runs_of(c))
    seen_align = set()
    for q in c["queries"][2:6]:
        r = ref_of(q, K)
        per_j = -(-r.u // 8)
        by_part = {}
        for t, km in enumerate(r.uniq):
            j, who = first_difference(km)
            if j is not None and j >= 8:
                by_part.setdefault(t // per_j, set()).add((j, who))
                seen_align.add((j, who, r.first[t] & 3))
        assert sorted(by_part) == list(range(8)), (r.u, sorted(by_part))
    assert seen_align == {(j, who, a) for j in range(8, 16) for who in ("fwd", "rc") for a in range(4)}


def test_one_call_sequences_cover_every_class():
    by = {}
    for cls, s in kc.ONE_CALL:
        by.setdefault(cls, []).append(s)
    assert sorted(by) == ["arg1024", "arg3072", "pinned", "read"]
    assert len(by["read"]) == 33 and all(len(s) <= 93 for s in by["read"])
    assert {first_difference(km) for s in by["read"] for km in [s[p:p + K] for p in range(len(s) - K + 1)]} >= set(SHAPE_OF)
    assert {a for _, _, a in kc.placements_in(by["read"]) if True} == {0, 1, 2, 3}
    for cls, lo, hi, arg in (("arg1024", 95, 1024, 1024), ("arg3072", 1025, 3072, 3072), ("pinned", 3073, 4126, 0)):
        assert len(by[cls]) >= 2 and all(lo <= len(s) <= hi and len(s) - K + 1 <= 4096 for s in by[cls]), cls
        assert kc.placements_in(by[cls]) >= kc.ALL_PLACEMENTS, cls
        for s in by[cls]:
            for thr in kc.THRESHOLDS[:2]:
                e = kc.expected_route([s], K, kc.H, kc.N_COLS, thr, {}, one_call=True)
                assert (e["instance"], e["k1_arg_bytes"], e["zero_copy"], e["one_launch"]) == ("k_kmerize_lds<31>", arg, 1, 0), (cls, len(s))
    for s in by["read"]:
        e = kc.expected_route([s], K, kc.H, kc.N_COLS, 1.0, {}, one_call=True)
        assert (e["instance"], e["k1_arg_bytes"], e["one_launch"]) == ("k_reads_fused", 96, 1)
    # the planted index: a k-mer hashed on the wrong strand misses column c; column c + 64 lacks one row of its latest-deciding k-mer
    pl = kc.planted("one_call")
    for c, (cls, s) in enumerate(kc.ONE_CALL):
        n, u, mk, hit, cnt = pl.expected(s, 1.0)
        t, row = pl.dropped[c]
        assert c in hit and c + 64 not in hit and cnt[hit.index(c)] == u, (c, cls)
        assert cls == "read" or first_difference(ref_of(s, K).uniq[t])[0] >= 8          # (the row taken out is a late-deciding shape's)
        wrong = [kc.signed_hash(kc.revcomp(kc.canonical(km)) if kc.revcomp(km) != km else km.lower(), sd) % kc.M for km in ref_of(s, K).uniq[t:t + 1] for sd in range(kc.H)]
        assert not all(x in pl.cols[c] for x in wrong), (c, "the other strand's rows must not be planted by chance")


def homopolymers(c):
    return {len(q) - c["k"] + 1 for q in c["queries"] if len(q) >= c["k"] and len(set(q)) == 1}


def test_dedupe_cases_reach_every_route():
    found = {}
    for c in CASES:
        if c["m"] != kc.M or c["h"] != kc.H:
            continue
        for inst in instances_of(c):
            found.setdefault(inst, set()).update(homopolymers(c))
        for q in c["queries"]:
            if len(q) >= c["k"] and len(set(q)) == 1:
                r = ref_of(q, c["k"])
                assert r.u == 1 and set(r.rep) == {0}
    # every size of the issue's grid on every instance that can take it: the read kernel holds 63 positions, a wavefront 64, the
    # LDS route 65 .. 4096 (eight parts: 256 .. 1024 positions in at most 32 queries), the global route anything
    sizes = set(kc.HOMOPOLYMER_SIZES)
    assert sizes == {1, 63, 64, 65, 256, 1024, 1025, 4096, 4097}
    lds1, lds8, wave = {n for n in sizes if 65 <= n <= 4096}, {256, 1024}, {1, 63, 64}
    want = {("k_reads_fused", 1): {1, 63}, ("k_kmerize_wave<31>", 1): wave, ("k_kmerize_lds<31>", 1): lds1, ("k_kmerize_lds<31>", 8): lds8,
            ("k_kmer_rows<31>", 1): sizes, ("k_kmerize_wave<0>", 1): wave, ("k_kmerize_lds<0>", 1): lds1, ("k_kmerize_lds<0>", 8): lds8,
            ("k_kmer_rows<0>", 1): sizes}
    for inst, need in want.items():
        assert found.get(inst, set()) >= need, (inst, sorted(need - found.get(inst, set())))
    # 256 and 1024 positions with ONE part: four passes of 256 threads (1024 queries), one full pass of 1024 (more than 32 queries)
    for name, block in (("lds_sorted", 256), ("lds_many", 1024), ("lds_many_k21", 1024)):
        c = kc.CASE_BY_NAME[name]
        assert homopolymers(c) >= {256, 1024} and all((e["k1_parts"], e["block"]) == (1, block) for _, _, _, e in runs_of(c)), name
    # period 2 and 3, both strands, lower case and N, in a case of every instance
    for name, k in (("reads", K), ("wave64", K), ("lds_dedupe", K), ("lds_sorted", K), ("lds_many", K), ("lds_parts8", K), ("global_dedupe", K),
                    ("wave_k21", 21), ("lds_k21", 21), ("lds_many_k21", 21), ("lds_parts8_k21", 21), ("global_k21", 21)):
        us = {}
        for q in kc.CASE_BY_NAME[name]["queries"]:
            r = ref_of(q, k)
            us[r.u] = us.get(r.u, 0) + (r.n > r.u)
            if len(q) == 2 * k and q[k:] == kc.revcomp(q[:k]) and q[k:] != q[:k]:
                rows = r.rows(kc.H, kc.M)
                assert r.uniq[0] == q[:k] and r.uniq[k] == q[k:] and rows[0] == rows[k], name      # two uniques, equal rows, in order
                us["strands"] = 1
            if len(q) == 3 * k and q[k:2 * k] == q[:k].lower():
                assert q[2 * k:] != q[:k] and "N" in q[2 * k:] and {q[:k], q[k:2 * k], q[2 * k:]} <= set(r.uniq)
                assert kc.revcomp(q[k:2 * k]) == q[k:2 * k][::-1]             # lower case complements to itself
                us["case"] = 1
        assert us.get(2) and us.get(3) and us.get("strands") and us.get("case"), (name, us)


def test_repeats_straddle_the_lane_pass_and_share_boundaries(planner):
    def reps(name, k=K):
        c = kc.CASE_BY_NAME[name]
        return c, {(r.n, p, r.rep[p]) for r in (ref_of(q, k) for q in c["queries"]) for p in range(r.n) if r.rep[p] != p and r.n - r.u <= 8}
    for name, k in (("lds_dedupe", K), ("global_dedupe", K), ("lds_k21", 21), ("global_k21", 21)):
        _, got = reps(name, k)
        assert {(200, 199, 0), (200, 63, 32), (200, 64, 33)} <= got, name          # positions 0 and n - 1; into lane 63; into lane 64
    assert (64, 63, 0) in reps("wave64")[1] and (64, 63, 32) in reps("wave64")[1] and (64, 63, 0) in reps("wave_k21", 21)[1]
    assert (63, 62, 0) in reps("reads")[1]
    # i / i + blockDim: the second pass of the workgroup
    for name, k, block, pair in (("lds_pass2", K, 1024, (1100, 1029, 5)), ("lds_pass2_k21", 21, 1024, (1100, 1029, 5)), ("lds_sorted", K, 256, (300, 261, 5))):
        c, got = reps(name, k)
        assert pair in got and pair[1] - pair[2] == block
        assert all(e["block"] == block and e["k1_parts"] == 1 for _, _, _, e in runs_of(c)), name
    # either side of a share boundary of parts = 8: 512 positions, shares of 64
    for name, k in (("lds_parts8", K), ("lds_parts8_k21", 21)):
        c, got = reps(name, k)
        assert {(512, 64, 10), (512, 100, 63), (512, 511, 0)} <= got and -(-512 // 8) == 64
        assert all(e["k1_parts"] == 8 for _, _, _, e in runs_of(c))


def test_fingerprint_collisions_and_wrapping_probe_chains(planner):
    for pairs, fp in ((kc.FP31_PAIRS, kc.fp31), (kc.FNV31_PAIRS, kc.fnv_fold), (kc.FNV21_PAIRS, kc.fnv_fold)):
        assert len(pairs) >= 3 and all(a != b and fp(a) == fp(b) and len(a) == len(b) for a, b in pairs)
    assert all(kc.fp31(a) != kc.fp31(b) for a, b in kc.FNV31_PAIRS) and all(kc.fnv_fold(a) != kc.fnv_fold(b) for a, b in kc.FP31_PAIRS)

    def holds(name, queries):
        have = kc.CASE_BY_NAME[name]["queries"]
        for q in queries:
            assert q in have, (name, q)
            k = kc.CASE_BY_NAME[name]["k"]
            r = ref_of(q, k)
            assert q[:k] != q[k:2 * k] and r.rep[2 * k] == 0 and r.pos_unique[k] == k != r.pos_unique[0]      # two uniques, the copy resolves
    holds("lds_dedupe", kc.abab(kc.FP31_PAIRS))              # kmer31_fingerprint: k_kmerize_lds<31>
    holds("lds_sorted", kc.abab(kc.FP31_PAIRS))
    holds("reads", kc.aba(kc.FP31_PAIRS))                    # ... and the read kernel's exact pairwise loop, without the weak flag
    holds("reads", kc.aba(kc.FNV31_PAIRS))                   # folded FNV-1a at k = 31: k_kmerize_wave<31> (the thresholded runs)
    holds("wave64", kc.aba(kc.FNV31_PAIRS))
    holds("global_dedupe", kc.abab(kc.FNV31_PAIRS))          # ... and k_kmer_insert<31>
    holds("wave_k21", kc.aba(kc.FNV21_PAIRS))                # folded FNV-1a at k = 21: wave<0>, LDS<0>, global<0>
    holds("lds_k21", kc.abab(kc.FNV21_PAIRS))
    holds("global_k21", kc.abab(kc.FNV21_PAIRS))
    # probe chains that wrap past the last slot: at least three k-mers at home there, table sizes by the route's own rule
    for name, last, fp, lds_route in (("lds_dedupe", kc.FP31_LAST, kc.fp31, True), ("lds_sorted", kc.FP31_LAST, kc.fp31, True), ("lds_k21", kc.FNV21_LAST, kc.fnv_fold, True),
                                      ("global_dedupe", kc.FNV31_LAST, kc.fnv_fold, False), ("global_k21", kc.FNV21_LAST, kc.fnv_fold, False)):
        c = kc.CASE_BY_NAME[name]
        k = c["k"]
        q = next(s for s in c["queries"] if len(s) == k * len(last) and sorted(s[i:i + k] for i in range(0, len(s), k)) == sorted(last))
        assert len(set(last)) == len(last) >= 3
        n = len(q) - k + 1
        inp = (len(c["queries"]), max(len(s) - k + 1 for s in c["queries"]), max(len(s) for s in c["queries"]))
        tab_mult = planner_k1(planner, *inp, False)["tab_mult"]
        slots = kc.k1_table_slots(n, tab_mult) if lds_route else kc.global_table_slots(n)
        assert slots <= 1024 and all(fp(km) & (slots - 1) == slots - 1 for km in last)
        tab = kc.replay_inserts(q, k, slots, fp)
        assert tab[slots - 1] == 0 and tab[0] is not None and q[tab[0]:tab[0] + k] in last and tab[0] > 0, (name, slots, tab[0])


def test_isolation_layout():
    for c in CASES:
        q, k = c["queries"], c["k"]
        if len(q) < 10 or c["name"] in ("reads", "reads_h1", "lds_sorted") or c["name"].startswith("m"):
            continue
        mid = len(q) // 2
        assert len(q[0]) < k and q[1] == "" and q[-1] == "" and len(q[-2]) < k, c["name"]
        assert any(s == "" for s in q[2:-2]) and any(0 < len(s) < k or k <= 2 for s in q[2:-2]) and q.count(q[2]) == 2, c["name"]
        assert abs(q.index("", 2) - mid) <= 2
    many = kc.CASE_BY_NAME["lds_sorted"]["queries"]
    assert many[3] == "" and len(many[-2]) == K - 1 and len(many[-1]) > 300 and max(len(s) for s in many[:3]) == K
    long_one = next(i for i in range(1024) if len(many[i]) - K + 1 == 400)
    assert len(many[long_one - 1]) < 200 and len(many[long_one + 1]) < 200 and len(set(many[long_one])) == 4          # one long query between short ones


def test_runtime_k_shapes_and_the_modulus_branches():
    assert {k & 3 for k in kc.RUNTIME_KS} == {0, 1, 2, 3} and set(kc.RUNTIME_KS) == {1, 2, 3, 4, 20, 23, 30, 32, 33}
    for k in kc.RUNTIME_KS:
        last = -(-k // 2) - 1
        js = kc.runtime_js(k)
        assert js[0] == 0 and js[-1] == last and (last < 2 or 0 < js[1] < last)
        want = {(j, who) for j in js for who in ("fwd", "rc")} | {(None, "tie")}
        assert {key for key, _ in kc.RUNTIME_SHAPES[k]} == want
        if k % 2 == 0:
            assert set(dict(kc.RUNTIME_SHAPES[k])[(None, "tie")]) <= set("ACGT")           # a true palindrome
        for suffix, inst in (("wave", "k_kmerize_wave<0>"), ("lds", "k_kmerize_lds<0>"), ("global", "k_kmer_rows<0>")):
            c = kc.CASE_BY_NAME["k%d_%s" % (k, suffix)]
            assert {i for i, _ in instances_of(c)} == {inst}, (k, suffix)
            got = {first_difference(q[p:p + k]) for q in c["queries"] for p in range(max(len(q) - k + 1, 0))}
            assert got >= want, (k, suffix, want - got)
    # D: a negative hash whose magnitude is a multiple of m (the a == 0 branch) and one that is not, for each m
    for m in (2, 7, kc.M):
        zero = other = 0
        for c in CASES:
            if c["m"] != m:
                continue
            for q in c["queries"][:80]:
                for km in ref_of(q, c["k"]).uniq:
                    for sd in range(c["h"]):
                        v = kc.signed_hash(kc.canonical(km), sd)
                        if v < 0:
                            zero += abs(v) % m == 0
                            other += abs(v) % m != 0
                            assert v % m == ((m - abs(v) % m) % m)
        assert zero and other, (m, zero, other)


# --------------------------------------------------------------------------------------------- (3) routes
@pytest.mark.parametrize("name", NAMES)
def test_every_run_takes_the_instance_it_is_built_for(planner, name):
    c = kc.CASE_BY_NAME[name]
    q, k, h = c["queries"], c["k"], c["h"]
    n, max_pos, max_len = len(q), max(max(len(s) - k + 1, 0) for s in q), max(len(s) for s in q)
    wv = -(-c["n_cols"] // 64)
    for thr, kw, built_for, e in runs_of(c):
        assert e["instance"] == built_for, (name, thr, kw, e)
        if e["one_launch"]:
            # reads_fusable, restated once more: k = 31, at most 63 positions, 2 <= h <= 4, exact or sparse counts, no forced route
            assert k == 31 and max_pos <= 63 and 2 <= h <= 4 and (thr == 1.0 or kw.get("sparse_counts")) and not kw.get("k1_global")
            continue
        p = planner_k1(planner, n, max_pos, max_len, bool(kw.get("k1_global")))
        assert p["route"] == e["k1_route"] and (p["route"] == kc.K1_WAVE or p["tab_mult"] == e["tab_mult"]), (name, p, e)
        ws = planner_want_sorted(planner, n, wv, max_pos, h, thr == 1.0)
        sort_block = planner.launch_host_sort_rows_block(max_pos, h)
        want = kc.NONE if not ws else kc.BY_K1 if p["route"] == kc.K1_LDS else kc.SORT1024 if sort_block == 1024 else kc.SORT256
        assert e["sorted_by"] == want, (name, thr, e["sorted_by"], want)
        if p["route"] == kc.K1_LDS:
            assert e["block"] in (64, 128, 256, 512, 1024) and (e["block"] >= max_pos or e["block"] == (256 if n >= 1024 else 1024))
            assert (e["k1_parts"] == 8) == (not ws and 256 <= max_pos <= e["block"] and n <= 32)
            assert p["lds"] <= 60 * 1024
    src = open(os.path.join(ROOT, "bigsi_amd", "csrc", "bigsi_kernels.hpp")).read()
    assert re.search(r"kSeqArgSmall = 1024, kSeqArgLarge = 3072, kSeqArgRead = 96;", src)
    assert (kc.ARG_READ, kc.ARG_SMALL, kc.ARG_LARGE) == (96, 1024, 3072)


def test_every_instance_is_reached():
    got = set()
    for c in CASES:
        got |= instances_of(c)
    assert got == {("k_reads_fused", 1), ("k_kmerize_wave<31>", 1), ("k_kmerize_wave<0>", 1), ("k_kmerize_lds<31>", 1), ("k_kmerize_lds<31>", 8),
                   ("k_kmerize_lds<0>", 1), ("k_kmerize_lds<0>", 8), ("k_kmer_rows<31>", 1), ("k_kmer_rows<0>", 1)}


def test_library_binds_the_position_hook_and_the_longer_route_record():
    from bigsi_amd import _lib
    fn = _lib.lib().bigsi_hip_batch_fetch_positions
    assert fn.restype == C.c_int and fn.argtypes == [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
    src = open(os.path.join(ROOT, "include", "bigsi_hip_testing.h")).read()
    assert re.search(r"int bigsi_hip_batch_fetch_positions\(bigsi_hip_batch \*b, uint32_t seq, uint32_t \*rep, uint32_t \*pos_unique, uint64_t capacity\);", src)
    assert [f for f, _ in _lib.RowAndPath._fields_][-2:] == ["k1_parts", "k1_arg_bytes"] and C.sizeof(_lib.RowAndPath) == 72
    buf = np.zeros(4, np.uint32)
    assert fn(None, 0, ptr(buf), ptr(buf), 4) == _lib.ERR_INVALID


# --------------------------------------------------------------------------------------------- (4) the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(CPU_LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(CPU_LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    return L


def twin_search(L, pl, seqs, thr):
    ix = C.c_void_p()
    assert L.bigsi_cpu_open(C.c_uint64(pl.m), C.c_uint64(kc.N_COLS), C.c_uint64(kc.N_COLS), C.c_uint32(pl.h), 0, C.byref(ix)) == 0
    try:
        ids, packed = pl.packed()
        assert L.bigsi_cpu_set_rows(ix, ptr(ids), C.c_uint64(ids.size), ptr(packed), C.c_uint64(packed.shape[1])) == 0, L.bigsi_cpu_last_error()
        data = [s.encode("ascii") for s in seqs]
        off = np.zeros(len(data) + 1, np.uint64)
        off[1:] = np.cumsum([len(d) for d in data])
        n = len(seqs)
        nk, nu, mk, ho = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
        cap = 128 * n + 64
        col, cnt = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        rc = L.bigsi_cpu_search_batch(ix, b"".join(data), ptr(off), C.c_uint32(n), C.c_uint32(pl.k), C.c_double(thr), C.c_uint32(0),
                                      ptr(nk), ptr(nu), ptr(mk), ptr(ho), ptr(col), ptr(cnt), C.c_uint64(cap))
        assert rc == 0, L.bigsi_cpu_last_error()
        return nk, nu, mk, ho, col, cnt
    finally:
        assert L.bigsi_cpu_close(ix) == 0


@pytest.mark.parametrize("name", ["one_call", "k31", "k21"] + ["k%d" % k for k in kc.RUNTIME_KS])
def test_cpu_twin_answers_the_planted_searches_as_the_reference_does(cpu, name):
    pl = kc.planted(name)
    assert 8 <= len(pl.seqs) <= 64
    if name == "k31":
        # the sample is chosen by name: all of set A, and of B the collision pairs of both fingerprints, both wrap queries, the
        # straddling repeats, both strands / lower case / N, and homopolymers
        assert kc.placements_in(pl.seqs) >= kc.ALL_PLACEMENTS
        have = set(pl.seqs)
        assert have >= set(kc.abab(kc.FP31_PAIRS) + kc.abab(kc.FNV31_PAIRS) + kc.aba(kc.FP31_PAIRS)[:2] + kc.aba(kc.FNV31_PAIRS)[:2])
        assert have >= {kc.homopolymer(n, K) for n in (1, 63, 64, 65, 256, 1024)}
        for last in (kc.FP31_LAST, kc.FNV31_LAST):
            assert any(len(s) == K * len(last) and sorted(s[i:i + K] for i in range(0, len(s), K)) == sorted(last) for s in have)
        reps = {(r.n, p, r.rep[p]) for r in (ref_of(s, K) for s in have) for p in range(r.n) if r.rep[p] != p and r.n - r.u <= 8}
        assert reps >= {(200, 199, 0), (200, 63, 32), (200, 64, 33), (512, 64, 10), (512, 100, 63), (300, 261, 5), (1024, 1023, 0), (64, 63, 0), (63, 62, 0)}
        assert any(len(s) == 2 * K and s[K:] == kc.revcomp(s[:K]) for s in have) and any(len(s) == 3 * K and s[K:2 * K] == s[:K].lower() for s in have)
    if name == "k21":
        have = set(pl.seqs)
        assert have >= set(kc.abab(kc.FNV21_PAIRS) + kc.aba(kc.FNV21_PAIRS)) | {kc.homopolymer(n, 21) for n in (1, 63, 64, 65, 256, 1024)}
        assert any(len(s) == 21 * 5 and sorted(s[i:i + 21] for i in range(0, len(s), 21)) == sorted(kc.FNV21_LAST) for s in have)
        reps = {(r.n, p, r.rep[p]) for r in (ref_of(s, 21) for s in have) for p in range(r.n) if r.rep[p] != p and r.n - r.u <= 8}
        assert reps >= {(200, 199, 0), (200, 63, 32), (200, 64, 33), (64, 63, 0), (1024, 1023, 0)}
        assert any(len(s) == 42 and s[21:] == kc.revcomp(s[:21]) for s in have) and any(len(s) == 63 and s[21:42] == s[:21].lower() for s in have)
    for thr in (1.0, 0.5):
        nk, nu, mk, ho, col, cnt = twin_search(cpu, pl, pl.seqs, thr)
        for i, s in enumerate(pl.seqs):
            n, u, want_mk, hit, counts = pl.expected(s, thr)
            a, b = int(ho[i]), int(ho[i + 1])
            assert (int(nk[i]), int(nu[i]), int(mk[i])) == (n, u, want_mk), (name, i, thr)
            assert col[a:b].tolist() == hit and cnt[a:b].tolist() == counts, (name, i, thr, len(s))
    # the build side of the twin sets exactly the reference's rows for every shape
    k = pl.k
    shapes = SHAPES if k == K else kc.RUNTIME_SHAPES.get(k, [])
    for _, s in shapes:
        out = np.zeros((kc.M + 7) // 8, np.uint8)
        assert cpu.bigsi_cpu_bloom(0, s.encode("ascii"), C.c_uint64(1), C.c_uint32(k), C.c_uint64(kc.M), C.c_uint32(kc.H), C.c_uint32(0), ptr(out)) == 0
        assert np.flatnonzero(np.unpackbits(out)[:kc.M]).tolist() == sorted(set(kc.kmer_rows(s, kc.H, kc.M))), s


# --------------------------------------------------------------------------------------------- (5) sensitivity
def _alignbyte(hi, lo, s):
    return (((hi << 32) | lo) >> (8 * s)) & 0xFFFFFFFF


def _bswap(x):
    return int.from_bytes(x.to_bytes(4, "little"), "big")


_staged = {}


def staged(seq):
    """the sequence and its complement as the kernels stage them: zero-padded, the complement 4 pad bytes in"""
    if seq not in _staged:
        raw = seq.encode("ascii")
        pad = lambda b: b + b"\0" * (48 - len(b) % 4)      # noqa: E731
        _staged[seq] = (pad(raw), pad(b"\0\0\0\0" + bytes(ord(kc.complement(chr(c))) for c in raw)))
    return _staged[seq]


def packed_canonical(seq, p, invert_word=None, tie_to_rc=False):
    """kmer31_words + kmer31_canonical_premix restated on Python integers: the 31-mer at position p of a sequence staged as
    little-endian words, its complement staged with 4 pad bytes in front; eight words cut out at the byte alignment, compared
    big-endian.  invert_word = i: the decision of word i is the wrong way round; tie_to_rc: a tie takes the reverse complement."""
    sw, cw = staged(seq)
    word = lambda buf, i: int.from_bytes(buf[4 * i:4 * i + 4], "little")      # noqa: E731
    d = [word(sw, (p >> 2) + i) for i in range(9)]
    wf = [_alignbyte(d[i + 1], d[i], p & 3) for i in range(8)]
    wf[7] &= 0x00FFFFFF
    base, sh = ((p + 31) >> 2) - 7, (p + 3) & 3
    e = [word(cw, base + i) for i in range(9)]
    x = [_alignbyte(e[8 - i], e[7 - i], sh) for i in range(8)]
    x[7] &= 0xFFFFFF00
    rc, decided = tie_to_rc, False
    for i in range(8):
        f = _bswap(wf[i])
        if not decided and f != x[i]:
            rc = (x[i] < f) != (i == invert_word)
            decided = True
    out = b"".join((_bswap(x[i]) if rc else wf[i]).to_bytes(4, "little") for i in range(8))
    return out[:31].decode("ascii")


def test_a_wrong_word_of_the_packed_compare_fails_set_a_at_every_alignment():
    cases = {"reads": kc.CASE_BY_NAME["reads"]["queries"][:66], "lds_shapes": kc.CASE_BY_NAME["lds_shapes"]["queries"],
             "arg1024": [s for cls, s in kc.ONE_CALL if cls == "arg1024"], "pinned": [s for cls, s in kc.ONE_CALL if cls == "pinned"][:1]}
    mutants = [dict(invert_word=i) for i in range(4)]
    shape_strings = set(SHAPE_OF.values())
    for name, queries in cases.items():
        wrong = {i: set() for i in range(len(mutants))}
        for q in queries:
            for p in range(max(len(q) - K + 1, 0)):
                km = q[p:p + K]
                want = kc.canonical(km)
                assert packed_canonical(q, p) == want, (name, p, km)
                # (a k-mer equal to its reverse complement has ONE canonical string: which side a tie takes cannot show in any row;
                # what the tie shapes pin is that a compare which finds no difference in eight words still emits the k-mer's bytes)
                assert packed_canonical(q, p, tie_to_rc=True) == want
                if km in shape_strings:
                    for i, kw in enumerate(mutants):
                        if packed_canonical(q, p, **kw) != want:
                            wrong[i].add(p & 3)
        for i, kw in enumerate(mutants):
            assert wrong[i] == {0, 1, 2, 3}, (name, kw, wrong[i])


def select_canonical(km, wrong_step=None, last_step=None):
    """RegKmer<31>::canonical_words restated: byte by byte against the complement of the mirrored byte, the first difference
    decides, select-only.  wrong_step = j: step j selects the wrong way round; last_step = j: the chain ends after step j."""
    rc = decided = False
    for j in range(len(km)):
        a, b = km[j], kc.complement(km[len(km) - 1 - j])
        take = (not decided) and a != b and (last_step is None or j <= last_step)
        if take:
            rc = (b < a) != (j == wrong_step)
        decided = decided or take
    return kc.revcomp(km) if rc else km


def test_a_wrong_step_of_the_select_chain_fails_the_shape_of_that_step():
    """the wave and the global route at k = 31 (the read batch's thresholded and forced-global runs, the 64-position queries)"""
    queries = kc.CASE_BY_NAME["reads"]["queries"][:66] + kc.CASE_BY_NAME["wave64"]["queries"]
    shape_of_string = {s: key for key, s in SHAPES}
    wrong = {j: set() for j in range(16)}
    cut = {j: set() for j in range(16)}
    for q in queries:
        for p in range(max(len(q) - K + 1, 0)):
            km = q[p:p + K]
            want = kc.canonical(km)
            assert select_canonical(km) == want
            if km in shape_of_string:
                for j in range(16):
                    if select_canonical(km, wrong_step=j) != want:
                        wrong[j].add(shape_of_string[km])
                    if select_canonical(km, last_step=j - 1) != want:
                        cut[j].add(shape_of_string[km])
    for j in range(16):
        # step j the wrong way round: exactly the two shapes decided at j; a chain that ends before step j: every shape the reverse
        # complement wins at j or later
        assert wrong[j] == {(j, "fwd"), (j, "rc")}, (j, wrong[j])
        assert cut[j] == {(i, "rc") for i in range(j, 16)}, (j, cut[j])
