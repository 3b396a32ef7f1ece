"""tests/presence_reference.py -- the reference the GPU suite compares bigsi_hip_batch_presence_hits with -- against the CPU twin
(bigsi_cpu_presence, include/bigsi_cpu.h), and its mirror of the piece geometry of k_presence_pieces / k_presence_expand on the
exact queries tests/test_gpu_presence_hits.py uses: a change to those constructions that loses a branch fails here, without a GPU."""
import ctypes as C

import numpy as np
import pytest

import presence_reference as pref
from raw_index import ptr
from test_cpu_twin import Index, cpu, pack      # noqa: F401 -- cpu is a fixture


def twin_and_oracle(cpu, m, n_cols, h, k, seed, draws, planted):
    """A twin index and a SynthOracle holding the same bits: the seeded synthetic fill plus `planted` = [(colour, sequence)]."""
    from oracle.ref_model import SynthOracle
    ix = Index(cpu, m, h, n_cols)
    ix.ok(cpu.bigsi_cpu_set_num_cols(ix.ix, C.c_uint64(n_cols)))
    ix.ok(cpu.bigsi_cpu_fill_synthetic(ix.ix, C.c_uint64(seed), C.c_uint64(0), C.c_uint32(draws)))
    orc = SynthOracle(seed, 0, m, n_cols, h, k, draws)
    for col, s in planted:
        blob, off = pack([s])
        ix.ok(cpu.bigsi_cpu_insert_kmers(ix.ix, C.c_uint64(col), blob, ptr(off), C.c_uint32(1), C.c_uint32(k)))
        orc.insert_kmers(col, s)
    return ix, orc


def twin_presence(cpu, ix, seq, k, colours):
    colours = np.ascontiguousarray(colours, dtype=np.uint32)
    n = max(len(seq) - k + 1, 0)
    out = np.zeros((colours.size, max(n, 1)), np.uint8)
    ix.ok(cpu.bigsi_cpu_presence(ix.ix, seq.encode(), C.c_uint64(len(seq)), C.c_uint32(k), ptr(colours), C.c_uint32(colours.size), ptr(out)))
    return [bytes(r[:n]).decode() for r in out]


@pytest.mark.parametrize("k,n_cols,h", [(31, 200, 3), (6, 200, 2), (31, 129, 1), (6, 1000, 4)])
def test_presence_strings_equal_the_cpu_twin(cpu, k, n_cols, h):
    """Repeats, N and lower case, a palindromic k-mer (even k), a k-mer beside its reverse complement, 1 / 16 / 17 positions; the
    columns at the word and pair edges and all columns at once.  The index is dense enough (one draw, small m) for the strings
    to be mixed, and pieces of the queries are planted so that long runs of ones occur too."""
    rng = np.random.default_rng(100 * k + h)
    a, b = pref.rand_seq(rng, 3 * k), pref.rand_seq(rng, 2 * k + 5)
    rc = a[:k + 7][::-1].translate(str.maketrans("ACGT", "TGCA"))
    queries = [a + a + b,                                           # repeats
               a[:k + 4] + "N" + b.lower() + a[:k + 2] + "nNa",      # N, lower case, a repeat of the head
               a[:k + 7] + rc,                                       # every k-mer of the head beside its reverse complement
               b[:k], b[:k + 15], b[:k + 16],                        # 1, 16, 17 positions
               b[:k - 1], ""]                                        # none
    if k == 6:
        queries.append("TTGAATTCAAGAATTCGG")                         # GAATTC is its own reverse complement, and occurs twice
        assert "GAATTC"[::-1].translate(str.maketrans("ACGT", "TGCA")) == "GAATTC"
    planted = [(0, a), (63 % n_cols, a[: 2 * k]), (64 % n_cols, b), (127 % n_cols, queries[1]), (128 % n_cols, a + b), (n_cols - 1, queries[2])]
    ix, orc = twin_and_oracle(cpu, 211, n_cols, h, k, 5 + h, 1, planted)
    edge = [c for c in (0, 63, 64, 127, 128, n_cols - 1) if c < n_cols]
    mixed = 0
    for q in queries:
        n = max(len(q) - k + 1, 0)
        pm = pref.position_map(q, k)
        kmers, uniq, rows = orc.per_kmer_rows(q)
        assert pm.size == n and [uniq[j] for j in pm] == kmers
        for cols in (edge, edge[::-1], np.arange(n_cols), rng.permutation(n_cols)[:37]):
            got = pref.presence_strings(orc, q, cols, rows)
            assert got == twin_presence(cpu, ix, q, k, cols), (q, list(cols)[:6])
            assert all(len(s) == n for s in got) and len(got) == len(cols)
            mixed += sum(1 for s in got if "0" in s and "1" in s)
        assert pref.presence_strings(orc, q, edge) == pref.presence_strings(orc, q, edge, rows)      # (rows computed inside)
    assert mixed > 100
    ix.close()


def test_presence_matrix_is_vectorised_over_colours(cpu):
    """All 16 385 columns of a 300-position query in one call: the same characters as one colour at a time."""
    k, n_cols = 31, 16385
    rng = np.random.default_rng(7)
    q = pref.rand_seq(rng, 330)
    ix, orc = twin_and_oracle(cpu, 97, n_cols, 2, k, 3, 1, [(8192, q[:200]), (n_cols - 1, q)])
    rows = orc.per_kmer_rows(q)[2]
    mat = pref.presence_matrix(orc, q, np.arange(n_cols), rows)
    assert mat.shape == (n_cols, 300) and mat.dtype == np.uint8
    cols = [0, 63, 64, 127, 128, 8191, 8192, 8193, n_cols - 2, n_cols - 1]
    assert [mat[c].tobytes().decode() for c in cols] == twin_presence(cpu, ix, q, k, cols)
    assert mat[n_cols - 1].tobytes() == b"1" * 300
    ix.close()


# ------------------------------------------------------------------------------------------------------- the piece geometry
def brute_classes(pm, pieces):
    """piece_classes restated position by position from the kernel's text: which lane holds what."""
    n, G = len(pm), min(pieces, 64)
    out = []
    for piece in range((n + 15) // 16):
        seg = [int(x) for x in pm[16 * piece:16 * piece + 16]]
        if any(seg[t] != seg[0] + t for t in range(len(seg))):
            out.append("listed")
            continue
        c, r = seg[0] // 16, seg[0] % 16
        first_of_group = piece - piece % G                     # the piece of the group's first lane: lanes hold chunk == their piece
        lo = "shuffle" if c >= first_of_group else "global"
        hi = "unused" if r == 0 else "shuffle" if first_of_group <= c + 1 < first_of_group + G else "global"
        out.append((lo, hi))
    return out


def test_piece_classes_on_small_maps():
    assert pref.pieces_for(1) == 1 and pref.pieces_for(16) == 1 and pref.pieces_for(17) == 2 and pref.pieces_for(1008) == 64
    assert pref.pieces_for(1024) == 64 and pref.pieces_for(1025) == 128
    pm = np.arange(40)
    assert [(p["listed"], p["cnt"], p["delta"], p["r"], p["lo"], p["hi"]) for p in pref.piece_classes(pm)] == \
        [(False, 16, 0, 0, "shuffle", "unused")] * 2 + [(False, 8, 0, 0, "shuffle", "unused")]
    pm = np.concatenate([np.arange(8), np.arange(8), np.arange(8, 24)])          # the map of per32
    got = pref.piece_classes(pm)
    assert got[0] == {"piece": 0, "listed": True, "cnt": 16}
    assert (got[1]["j0"], got[1]["delta"], got[1]["r"], got[1]["sub"], got[1]["G"], got[1]["lo"], got[1]["hi"]) == (8, 1, 8, 1, 2, "shuffle", "shuffle")
    assert pref.class_names(pm) == {"listed": 1, "lo_shuffle": 1, "hi_shuffle": 1, "delta_eq_sub_pos": 1, "delta_pos": 1}
    # the same map inside a call whose longest hit-bearing query is longer: same lanes within the wider group
    assert pref.piece_classes(pm, 64)[1]["sub"] == 1


ALL_RUN_CLASSES = {"lo_shuffle", "lo_global", "hi_shuffle", "hi_global", "hi_unused", "delta_eq_sub_plus_1", "delta_eq_sub_pos", "delta_pos", "tail"}


def test_the_gpu_tests_queries_reach_every_branch():
    """The constructions of tests/test_gpu_presence_hits.py section b, class by class (K = 31, random ACGT)."""
    qs = pref.long_queries()
    k = pref.K
    pm = {name: pref.position_map(s, k) for name, s in qs.items()}
    assert {name: len(v) for name, v in pm.items()} == {
        "rep128": 1870, "rep256": 3578, "rep32": 360, "ac500": 470, "ac330": 300, "read61": 31, "rep1008": 1008, "rep1024": 1024,
        "rep64": 64, "rep56": 56, "per32": 32, "per16": 16, "run17": 17, "run16": 16, "run9": 9, "run1": 1, "nohits": 1970, "per300": 300, "per1070": 1070}
    for name, v in pm.items():              # piece_classes == the position-by-position restatement, in their own call and in the widest
        for pieces in (pref.pieces_for(len(v)), 256):
            got = [("listed" if p["listed"] else (p["lo"], p["hi"])) for p in pref.piece_classes(v, pieces)]
            assert got == brute_classes(v, pieces), (name, pieces)
    c128 = pref.class_names(pm["rep128"])
    assert pref.pieces_for(1870) == 128 and ALL_RUN_CLASSES <= set(c128) and c128["listed"] == 2, c128
    c256 = pref.class_names(pm["rep256"])
    # (the second A: delta == 66 > every sub, so lo and hi by global load; B's unique indices lie 1024 = 64 x 16 behind its positions:
    # r == 0 with delta == 64, the chunk always in the wavefront before)
    assert pref.pieces_for(3578) == 256 and {"lo_shuffle", "lo_global", "hi_global", "hi_unused", "r0_lo_global", "tail"} <= set(c256), c256
    assert c256["listed"] == 2 and c256["r0_lo_global"] >= 90 and c256["hi_global"] >= 60
    c32 = pref.class_names(pm["rep32"])
    assert pref.pieces_for(360) == 32 and {"lo_shuffle", "hi_shuffle", "hi_unused", "delta_pos", "listed", "tail"} <= set(c32), c32
    assert "lo_global" not in c32 and "hi_global" not in c32            # one group per hit: nothing lies in another wavefront
    for name in ("ac500", "ac330"):
        c = pref.class_names(pm[name])
        assert c["listed"] >= 10 and {"hi_shuffle", "delta_pos", "tail"} <= set(c), (name, c)
    for name, pieces in (("rep1008", 64), ("rep1024", 64), ("rep64", 4), ("rep56", 4), ("per32", 2), ("per16", 1), ("run16", 1), ("run17", 2)):
        assert pref.pieces_for(len(pm[name])) == pieces, name
    for name in ("rep1008", "rep1024"):
        c = pref.class_names(pm[name])
        assert {"lo_shuffle", "hi_shuffle", "delta_pos", "listed"} <= set(c) and "lo_global" not in c, (name, c)
    assert {"listed", "delta_pos", "hi_shuffle"} <= set(pref.class_names(pm["rep64"]))
    assert {"listed", "delta_pos", "tail"} <= set(pref.class_names(pm["rep56"]))
    assert pref.class_names(pm["per32"]) == {"listed": 1, "lo_shuffle": 1, "hi_shuffle": 1, "delta_eq_sub_pos": 1, "delta_pos": 1}
    assert pref.class_names(pm["per16"]) == {"listed": 1}
    assert pref.class_names(pm["run9"]) == {"tail": 1, "lo_shuffle": 1, "hi_unused": 1}
    # 20 unique k-mers: 2 chunks of presence bits under 32 and 128 pieces
    for name, pieces, need in (("per300", 32, {"listed", "lo_shuffle", "hi_shuffle", "hi_unused", "delta_eq_sub_pos", "tail"}),
                               ("per1070", 128, {"listed", "lo_shuffle", "lo_global", "hi_shuffle", "hi_global", "hi_unused", "tail_listed"})):
        assert int(pm[name].max()) + 1 == 20 and pref.pieces_for(len(pm[name])) == pieces and need <= set(pref.class_names(pm[name])), name
    # in the widest call (256 pieces per hit) the shorter queries keep their lanes: sub = piece & 63
    assert pref.class_names(pm["rep128"], 256) == c128
