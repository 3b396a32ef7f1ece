"""Group association without a GPU: the host planner plan_associate (csrc/bigsi_launch.hpp, compiled by g++) against a plain Python
restatement (tests/associate_ref.py), the CPU twin bigsi_cpu_associate against the numpy reference on the planted indexes the GPU tests
use, the conditions those indexes must hold so that no GPU comparison passes vacuously, the host layer (bigsi_amd/associate.py:
associate_plan on classify_plan, the 2x2 tables, the statistics against exact fractions, TSV / JSON, min_af), what BIGSI.associate and
the command line decide before any device call, the ABI lists, and a stand-alone sanitized program over the planner and the twin."""
import ctypes as C
import json
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import associate_ref as R
import tally_ref as T
from conftest import ROOT
from raw_index import ptr

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
WIDTHS = (1, 63, 64, 65, 127, 129, 200, 775)
QUERY_COUNTS = (1, 3, 63, 64, 65, R.QUERIES - 1, R.QUERIES, R.QUERIES + 1)


def width_case(n_cols):
    """the planted index of a width case: 5 queries; the two widths the conditions are asserted on have 65"""
    return T.planted(n_cols, 65, seed=65) if n_cols in R.CONDITION_WIDTHS else T.planted(n_cols, 5)


def same(got, want, what):
    """(counts, info) pairs, bit for bit"""
    (gc, gi), (wc, wi) = got, want
    assert gc.dtype == wc.dtype == np.uint32 and gc.shape == wc.shape and gi.dtype == wi.dtype == R.INFO_DTYPE, what
    bad = np.flatnonzero((gc != wc).any(axis=1) | (gi != wi))
    assert bad.size == 0, (what, bad[:4], [(tuple(gi[i]), gc[i].tolist()) for i in bad[:3]], [(tuple(wi[i]), wc[i].tolist()) for i in bad[:3]])


# --------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("associate_host") / "libassociate_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "associate_host.cpp")])
    lib = C.CDLL(so)
    lib.associate_host_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    return lib


def compiled_plan(lib, n_seqs, wv, n_groups):
    out = np.zeros(8, np.uint64)
    lib.associate_host_plan(n_seqs, wv, n_groups, ptr(out))
    return dict(zip(("block", "grid", "mask_grid", "lds_bytes", "passes", "mask_bytes", "too_large", "bad_groups"), (int(x) for x in out)))


def test_constants_are_the_restated_ones(plan_lib):
    c = np.zeros(7, np.uint64)
    plan_lib.associate_host_constants(ptr(c))
    assert [int(x) for x in c] == [R.BLOCK, R.MAX_GROUPS, R.NONE, R.NONE, R.QUERIES, R.GROUP_BLOCK, T.CHUNK_SEQS]
    header = open(os.path.join(ROOT, "include", "bigsi_hip_associate.h")).read()
    classify_header = open(os.path.join(ROOT, "include", "bigsi_hip_classify.h")).read()
    assert "#define BIGSI_ASSOCIATE_NONE 0xFFFFFFFFu" in header and "#define BIGSI_ASSOCIATE_MAX_GROUPS 64u" in header
    assert "#define BIGSI_CLASSIFY_NONE 0xFFFFFFFFu" in classify_header          # BIGSI_ASSOCIATE_NONE == BIGSI_CLASSIFY_NONE: classify_bad_column serves both
    from bigsi_amd import associate, classify
    assert (associate.NONE, associate.MAX_GROUPS, associate.INFO_FIELDS) == (R.NONE, R.MAX_GROUPS, R.INFO_FIELDS) and associate.INFO_DTYPE == R.INFO_DTYPE
    assert associate.NONE == classify.NONE
    fields = re.search(r"typedef struct bigsi_hip_associate_info \{(.*?)\}", header, re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))) == R.INFO_FIELDS


def test_plan_associate_against_restatement(plan_lib):
    for n_seqs in (0, 1, 3, 4, 5, 4095, 4096, 4 * 0x7FFFFFFF, 4 * 0x7FFFFFFF + 1, 1 << 40):
        for wv in (1, 3, 4, 5, 13, 1563, 9375, 1 << 26, 1 << 34):
            for n_groups in (0, 1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 4096, 1 << 33):
                p = compiled_plan(plan_lib, n_seqs, wv, n_groups)
                assert p == R.plan_associate(n_seqs, wv, n_groups), (n_seqs, wv, n_groups)
                assert p["grid"] == -(-n_seqs // 4) and p["bad_groups"] == (not 1 <= n_groups <= 64)
                assert (p["too_large"] != 0) == (n_seqs > 4 * 0x7FFFFFFF or wv > 4 * 0x7FFFFFFF)
                if not p["bad_groups"]:
                    assert p["passes"] == -(-n_groups // 8) and p["mask_bytes"] == n_groups * wv * 8
    # the figures the header quotes: 64 groups at 100 k and 600 k columns
    assert compiled_plan(plan_lib, 1, 1563, 64)["mask_bytes"] == 800256 and compiled_plan(plan_lib, 1, 9375, 64)["mask_bytes"] == 4800000
    assert compiled_plan(plan_lib, 1, 1, 64)["lds_bytes"] == 576


# --------------------------------------------------------------------------------------------- the reference's own conditions
@pytest.mark.parametrize("n_cols", R.CONDITION_WIDTHS)
def test_cases_cannot_pass_vacuously(n_cols):
    """on the very planted indexes, layouts and thresholds the GPU cases run"""
    p = width_case(n_cols)
    thr, i, e = p.edge_threshold()
    assert 0 < thr < 1 and T.min_kmers(int(p.us[i]), thr) == int(p.counts[i, e]) < p.us[i]
    R.check_conditions(p, R.dense_case(n_cols))
    g, n_groups = R.layout("two", n_cols)
    assert n_groups == 2 and g[63] == R.NONE and g[0] == g[64] == 0 and g[1] == g[65] == 1 and (g == R.NONE).sum() == 1
    g, n_groups = R.layout("full64", n_cols)
    assert n_groups == 64 and g.max() == 63 and g[64] == 0 and (g != R.NONE).all()
    assert (-(-n_cols // 64)) % 2 == (0 if n_cols == 200 else 1)          # 775 columns: an odd number of result words, a pad word behind them


def test_group_counts_of_is_the_definition():
    """a second, vectorised statement of the definition over the whole counts matrix"""
    for p in (width_case(200), R.dense_case(200)):
        for name in R.LAYOUTS:
            g, n_groups = R.layout(name, 200)
            for thr in R.thresholds(p) + (-0.5,):
                counts, info = R.group_counts_of(p.us, p.counts, thr, g, n_groups)
                mk = np.array([T.min_kmers(int(u), thr) for u in p.us], np.int64)
                hit = (p.counts >= mk[:, None]) & (p.us > 0)[:, None]
                per = np.stack([(hit & (g == x)[None, :]).sum(axis=1) for x in range(n_groups)], axis=1)
                assert np.array_equal(counts, per) and np.array_equal(info["samples_hit"], hit.sum(axis=1))
                assert np.array_equal(info["grouped_hit"], (hit & (g != R.NONE)[None, :]).sum(axis=1))
                assert np.array_equal(info["num_unique"], p.us) and np.array_equal(info["min_kmers"], np.where(p.us > 0, mk, 0))
        assert all(np.array_equal(a, b) for a, b in zip(R.group_counts_of(p.us, p.counts, -0.5, g, n_groups), R.group_counts_of(p.us, p.counts, 0.0, g, n_groups)))


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    L.bigsi_cpu_associate.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    L.bigsi_cpu_associate.restype = C.c_int32
    return L


def twin_index(L, p, h=T.H):
    from bigsi_amd._lib import Info
    ix = C.c_void_p()
    assert L.bigsi_cpu_open(C.c_uint64(T.M), C.c_uint64(p.n_cols), C.c_uint64(p.n_cols), C.c_uint32(h), 0, C.byref(ix)) == 0
    inf = Info()
    assert L.bigsi_cpu_get_info(ix, C.byref(inf)) == 0
    rows = p.junk_rows(int(inf.row_stride_bytes))
    ids = np.arange(T.M, dtype=np.uint64)
    assert L.bigsi_cpu_set_rows(ix, ptr(ids), C.c_uint64(T.M), ptr(rows), C.c_uint64(rows.shape[1])) == 0, L.bigsi_cpu_last_error()
    return ix


def preset(n_seqs, n_groups):
    """output buffers preset to 0xAB, a guard entry behind each"""
    counts = np.zeros((n_seqs + 1, n_groups), np.uint32)
    info = np.zeros(n_seqs + 1, R.INFO_DTYPE)
    counts.view(np.uint8)[:] = 0xAB
    info.view(np.uint8)[:] = 0xAB
    return counts, info


def guards_hold(counts, info):
    return counts[-1].tobytes() == b"\xab" * (4 * counts.shape[1]) and info[-1].tobytes() == b"\xab" * 16


def untouched(out):
    counts, info = out
    return counts.tobytes() == b"\xab" * counts.nbytes and info.tobytes() == b"\xab" * info.nbytes


def twin_associate(L, ix, seqs, thr, g, n_groups, n_entries=None):
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(seqs)
    counts, info = preset(len(seqs), max(n_groups, 1))
    rc = L.bigsi_cpu_associate(ix, blob, ptr(off), len(seqs), T.K, thr, ptr(g), g.size if n_entries is None else n_entries, n_groups, ptr(counts), ptr(info))
    assert guards_hold(counts, info)
    return rc, (counts[:-1], info[:-1])


def part(want, sel):
    return want[0][sel], want[1][sel]


@pytest.mark.parametrize("n_cols", WIDTHS)
def test_twin_against_numpy(cpu, n_cols):
    p = width_case(n_cols)
    sel = slice(0, 5) if n_cols not in R.CONDITION_WIDTHS else slice(None)
    ix = twin_index(cpu, p)
    for name in R.LAYOUTS:
        g, n_groups = R.layout(name, n_cols)
        for thr in R.thresholds(p):
            rc, got = twin_associate(cpu, ix, p.seqs[sel], thr, g, n_groups)
            assert rc == 0, cpu.bigsi_cpu_last_error()
            same(got, part(R.planted_counts(p, thr, name), sel), (n_cols, name, thr))
    rc, got = twin_associate(cpu, ix, p.seqs[sel], -1.0, g, n_groups)
    same(got, part(R.planted_counts(p, 0.0, name), sel), (n_cols, "a threshold below 0"))
    assert cpu.bigsi_cpu_close(ix) == 0


@pytest.mark.parametrize("n_cols", R.CONDITION_WIDTHS)
def test_twin_on_the_dense_case(cpu, n_cols):
    p = R.dense_case(n_cols)
    ix = twin_index(cpu, p)
    for name in R.LAYOUTS:
        g, n_groups = R.layout(name, n_cols)
        for thr in (1.0, 0.0):
            rc, got = twin_associate(cpu, ix, p.seqs, thr, g, n_groups)
            assert rc == 0, cpu.bigsi_cpu_last_error()
            same(got, R.planted_counts(p, thr, name), ("dense", n_cols, name, thr))
    assert cpu.bigsi_cpu_close(ix) == 0


def test_twin_refusals(cpu):
    p = T.planted(65, 5)
    g, n_groups = R.layout("edges", 65)
    ix = twin_index(cpu, p)
    for thr, gg, n_entries, groups in ((1.5, g, None, n_groups), (float("nan"), g, None, n_groups), (1.0, g, 64, n_groups), (1.0, g, 66, n_groups), (1.0, g, None, 0),
                                       (1.0, g, None, 65), (1.0, g, None, 7)):          # (7 groups: the last column's id, 7, is out of range)
        rc, out = twin_associate(cpu, ix, p.seqs, thr, gg, groups, n_entries)
        assert rc == ERR_INVALID and untouched(out) and cpu.bigsi_cpu_last_error(), (thr, n_entries, groups)
    assert b"group_of[64]" in cpu.bigsi_cpu_last_error()
    twin_associate(cpu, ix, p.seqs, 1.0, g, 65)
    assert b"BIGSI_ASSOCIATE_MAX_GROUPS" in cpu.bigsi_cpu_last_error()
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(p.seqs)
    counts, info = np.zeros((5, n_groups), np.uint32), np.zeros(5, R.INFO_DTYPE)
    call = cpu.bigsi_cpu_associate
    tail = (ptr(counts), ptr(info))
    for args in ((None, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups) + tail, (ix, blob, None, 5, T.K, 1.0, ptr(g), 65, n_groups) + tail,
                 (ix, blob, ptr(off), 5, T.K, 1.0, None, 65, n_groups) + tail, (ix, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, None, ptr(info)),
                 (ix, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, ptr(counts), None),
                 (ix, blob, ptr(off), 0, T.K, 1.0, ptr(g), 65, n_groups) + tail, (ix, blob, ptr(off), 5, 0, 1.0, ptr(g), 65, n_groups) + tail):
        assert call(*args) == ERR_INVALID and cpu.bigsi_cpu_last_error()
    down = off.copy()
    down[2] = down[1] - 1
    assert call(ix, blob, ptr(down), 5, T.K, 1.0, ptr(g), 65, n_groups, *tail) == ERR_INVALID
    assert cpu.bigsi_cpu_close(ix) == 0
    empty = C.c_void_p()
    assert cpu.bigsi_cpu_open(C.c_uint64(64), C.c_uint64(0), C.c_uint64(8), C.c_uint32(3), 0, C.byref(empty)) == 0
    assert call(empty, blob, ptr(off), 5, T.K, 1.0, ptr(g), 0, n_groups, *tail) == ERR_STATE
    assert cpu.bigsi_cpu_close(empty) == 0


# --------------------------------------------------------------------------------------------- the host layer
def test_associate_plan_on_classify_plan():
    from bigsi_amd import associate, classify
    from bigsi_amd.graph.metadata import DELETION_SPECIAL_SAMPLE_NAME as GONE
    names = ["a", "b", GONE, "c", "d", "e"]
    groups = {"x": ["d", "a"], "y": ["c"]}
    g, gn, sizes = associate.associate_plan(names, groups)
    want, want_names = classify.classify_plan(names, groups)
    assert g.dtype == np.uint32 and g.tolist() == want.tolist() == [0, R.NONE, R.NONE, 1, 0, R.NONE] and gn == want_names == ["x", "y"] and sizes.tolist() == [2, 1]
    # others: every unlisted LIVE sample in one more group; a deleted sample stays in none and in no size
    g, gn, sizes = associate.associate_plan(names, groups, others="rest")
    assert g.tolist() == [0, 2, R.NONE, 1, 0, 2] and gn == ["x", "y", "rest"] and sizes.tolist() == [2, 1, 2] and sizes.sum() == 5
    # classify_plan's refusals, unchanged
    for bad, err in (({"x": ["a"], "y": ["a"]}, ValueError), ({"x": []}, ValueError), ({}, ValueError), ({GONE: ["a"]}, ValueError),
                     ({"x": ["nobody"]}, KeyError), ({"x": [GONE]}, KeyError), ("x", TypeError)):
        with pytest.raises(err):
            associate.associate_plan(names, bad, others="rest")
    for others, err in (("x", ValueError), (GONE, ValueError), (5, TypeError)):
        with pytest.raises(err):
            associate.associate_plan(names, groups, others=others)
    many = ["s%d" % i for i in range(66)]
    g, gn, sizes = associate.associate_plan(many, [(s, "g" + s) for s in many[:64]])
    assert len(gn) == 64 and sizes.tolist() == [1] * 64
    with pytest.raises(ValueError, match="at most 64"):
        associate.associate_plan(many, [(s, "g" + s) for s in many[:65]])
    with pytest.raises(ValueError, match="at most 64"):
        associate.associate_plan(many, [(s, "g" + s) for s in many[:64]], others="rest")


# (a, b, c, d): the cases the feature names first, then zero margins of every kind, then ordinary tables, small and large
TABLES = [(10, 0, 0, 10), (7, 7, 7, 7), (1, 1, 1, 1),
          (0, 0, 0, 0), (0, 0, 5, 9), (4, 6, 0, 0), (0, 5, 0, 9), (5, 0, 9, 0), (0, 0, 0, 3), (3, 0, 0, 0), (0, 7, 0, 0), (0, 0, 7, 0),
          (0, 10, 10, 0), (3, 1, 2, 8), (1, 0, 0, 1), (12, 5, 7, 30), (499, 1, 3, 497), (50000, 1, 17, 49982), (123456789, 987654321, 555555555, 333333333)]


def test_statistics_against_exact_fractions():
    from bigsi_amd import associate
    for a, b, c, d in TABLES:
        n_g, rest, hit, total = a + b, c + d, a + c, a + b + c + d
        den = n_g * rest * hit * (total - hit)
        chi2 = float(Fraction(total * (a * d - b * c) ** 2, den)) if den else 0.0
        want = (float(Fraction(a, n_g)) if n_g else 0.0, math.log2(float(Fraction((2 * a + 1) * (2 * d + 1), (2 * b + 1) * (2 * c + 1)))), chi2,
                math.erfc(math.sqrt(chi2 / 2)))
        got = associate.statistics((a, b, c, d))
        assert got == want and all(type(x) is float for x in got), ((a, b, c, d), got, want)
    assert associate.statistics((10, 0, 0, 10))[2] == 20.0
    assert all(associate.statistics(t)[2:] == (0.0, 1.0) for t in TABLES[1:12])          # a = b = c = d and every zero margin
    assert associate.statistics((0, 10, 10, 0))[2] == 20.0 and associate.statistics((10, 0, 0, 10))[1] == -associate.statistics((0, 10, 10, 0))[1] > 0
    # the same with numpy integers: no 64-bit overflow, no numpy floats
    assert associate.statistics(tuple(np.uint32(x) for x in (4000000000, 1, 2, 4000000000))) == associate.statistics((4000000000, 1, 2, 4000000000))


def _case():
    """three records over groups A (4 samples), B (3), C (0: legal at the C boundary, and here): counts, info, sizes"""
    counts = np.array([[4, 0, 0], [2, 1, 0], [0, 0, 0], [4, 3, 0], [1, 3, 0]], np.uint32)
    info = np.zeros(5, R.INFO_DTYPE)
    info[:] = [(9, 9, 5, 4), (40, 16, 3, 3), (0, 0, 0, 0), (12, 0, 8, 7), (7, 7, 4, 4)]
    return counts, info, [4, 3, 0]


def test_tables_result_and_text():
    from bigsi_amd import associate
    counts, info, sizes = _case()
    tabs = associate.tables(counts, info, sizes)
    assert tabs[0] == [(4, 0, 0, 3), (0, 3, 4, 0), (0, 0, 4, 3)] and tabs[1] == [(2, 2, 1, 2), (1, 2, 2, 2), (0, 0, 3, 4)] and tabs[3][0] == (4, 0, 3, 0)
    assert all(type(x) is int and x >= 0 for rec in tabs for t in rec for x in t) and all(sum(t) == 7 for rec in tabs for t in rec)
    gn = ["A", "B\tb", "C"]
    res = associate.result(counts, info, gn, sizes)
    assert list(res) == ["groups", "sizes", "total", "records", "dropped"] and (res["groups"], res["sizes"], res["total"], res["dropped"]) == (gn, [4, 3, 0], 7, 0)
    assert [r["index"] for r in res["records"]] == [0, 1, 2, 3, 4]
    r = res["records"][0]
    assert (r["num_kmers"], r["min_kmers"], r["samples_hit"], r["grouped_hit"]) == (9, 9, 5, 4) and list(r["groups"]) == gn
    for name, t in zip(gn, tabs[0]):
        prevalence, log2_odds, chi2, p = associate.statistics(t)
        assert r["groups"][name] == {"hit": t[0], "prevalence": prevalence, "log2_odds": log2_odds, "chi2": chi2, "p": p}
    assert r["groups"]["A"]["chi2"] == 7.0 and r["groups"]["A"]["prevalence"] == 1.0 and r["groups"]["C"] == {"hit": 0, "prevalence": 0.0, "log2_odds": math.log2(7 / 9), "chi2": 0.0, "p": 1.0}
    ids = ["u0", "u\n1", "u2", "u3", "u4"]
    assert json.loads(associate.to_json(res, ids)) == dict(res, records=[dict({"name": n}, **x) for n, x in zip(ids, res["records"])])
    assert json.loads(associate.to_json(res))["records"] == res["records"]
    lines = associate.to_tsv(res, ids).split("\n")
    assert lines[0] == "name\tnum_kmers\tsamples_hit\t" + "\t".join("%s:%s" % (g, c) for g in ("A", "B b", "C") for c in ("hit", "prevalence", "log2_odds", "chi2", "p"))
    assert len(lines) == 7 and lines[-1] == "# dropped\t0" and lines[2].startswith("u 1\t40\t3\t2\t0.5\t")
    for line, rec in zip(lines[1:6], res["records"]):
        cells = line.split("\t")
        assert len(cells) == 3 + 5 * 3
        for j, g in enumerate(gn):
            s = rec["groups"][g]
            assert cells[3 + 5 * j:8 + 5 * j] == [str(s["hit"]), repr(s["prevalence"]), repr(s["log2_odds"]), repr(s["chi2"]), repr(s["p"])]
            assert [float(x) for x in cells[4 + 5 * j:8 + 5 * j]] == [s["prevalence"], s["log2_odds"], s["chi2"], s["p"]]          # repr round-trips
    assert associate.result(np.zeros((0, 3), np.uint32), np.zeros(0, R.INFO_DTYPE), gn, sizes) == {"groups": gn, "sizes": [4, 3, 0], "total": 7, "records": [], "dropped": 0}


def test_min_af_bookkeeping():
    from bigsi_amd import associate
    counts, info, sizes = _case()          # H / T = 4/7, 3/7, 0, 1, 4/7
    gn = ["A", "B", "C"]
    full = associate.result(counts, info, gn, sizes)
    for f, kept in ((None, [0, 1, 2, 3, 4]), (0.0, [0, 1, 2, 3, 4]), (0.01, [0, 1, 4]), (0.42, [0, 1, 4]), (0.43, []), (0.5, [])):
        res = associate.result(counts, info, gn, sizes, min_af=f)
        assert [r["index"] for r in res["records"]] == kept and res["dropped"] == 5 - len(kept), f
        assert res["records"] == [full["records"][i] for i in kept]
        assert associate.to_tsv(res, ["u%d" % i for i in range(5)]).split("\n")[-1] == "# dropped\t%d" % (5 - len(kept))
        assert [x.split("\t")[0] for x in associate.to_tsv(res, ["u%d" % i for i in range(5)]).split("\n")[1:-1]] == ["u%d" % i for i in kept]
    for bad in (-0.1, 0.51, float("nan")):
        with pytest.raises(ValueError):
            associate.result(counts, info, gn, sizes, min_af=bad)


class _FakeIndex(object):
    def __init__(self):
        self.asked = None

    def associate(self, seqs, groups, threshold=1.0, others=None, min_af=None):
        from bigsi_amd import associate
        self.asked = (list(seqs), list(groups), threshold, others, min_af)
        counts, info, sizes = _case()
        return associate.result(counts[:2], info[:2], ["A", "B", "C"], sizes, min_af)


def test_cli_parsing_text_and_refusals(tmp_path, capsys):
    from bigsi_amd import associate
    from bigsi_amd.__main__ import associate_text, build_parser, main
    p = build_parser()[0]
    a = p.parse_args(["associate", "unitigs.fasta", "--groups", "g.tsv", "-c", "c.yaml"])
    assert (a.cmd, a.fasta, a.groups, a.threshold, a.others, a.min_af, a.format, a.config) == ("associate", "unitigs.fasta", "g.tsv", 1.0, None, None, "tsv", "c.yaml")
    a = p.parse_args(["associate", "u.fa", "--groups", "g.tsv", "-t", "0.4", "--others", "rest", "--min-af", "0.05", "--format", "json"])
    assert (a.threshold, a.others, a.min_af, a.format) == (0.4, "rest", 0.05, "json")
    for argv in (["associate"], ["associate", "u.fa"], ["associate", "u.fa", "--groups", "g", "--min-af", "x"], ["associate", "u.fa", "--groups", "g", "--format", "csv"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    p.format_help()
    ix = _FakeIndex()
    text = associate_text(ix, [("q0", "ACGT"), ("q1", "TT")], [("s4", "A")], 0.5, "rest", 0.1)
    assert ix.asked == (["ACGT", "TT"], [("s4", "A")], 0.5, "rest", 0.1)
    counts, info, sizes = _case()
    want = associate.result(counts[:2], info[:2], ["A", "B", "C"], sizes, 0.1)
    assert text == associate.to_tsv(want, ["q0", "q1"]) and text.split("\n")[1].startswith("q0\t9\t5\t4\t1.0\t")
    assert json.loads(associate_text(ix, [("q0", "ACGT"), ("q1", "TT")], [("s4", "A")], fmt="json"))["records"][0]["name"] == "q0"
    # refused before any device call: --sharded, a threshold above 1, --min-af out of range, a groups file that cannot be read or names a sample twice
    good, twice = tmp_path / "g.tsv", tmp_path / "twice.tsv"
    good.write_text("s0\tx\ns1\ty\n")
    twice.write_text("s0\tx\ns0\ty\n")
    for argv, words in ((["associate", "u.fa", "--groups", str(good), "--sharded"], ("--sharded", "associate")), (["associate", "u.fa", "--groups", str(good), "-t", "1.5"], ("threshold",)),
                        (["associate", "u.fa", "--groups", str(good), "--min-af", "0.6"], ("--min-af",)),
                        (["associate", "u.fa", "--groups", str(tmp_path / "missing.tsv")], ("--groups",)), (["associate", "u.fa", "--groups", str(twice)], ("two groups",))):
        with pytest.raises(SystemExit):
            main(argv)
        err = capsys.readouterr().err
        assert all(w in err for w in words), (argv, err)


def test_associate_checks_its_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    g = {"x": ["a"]}
    for seqs, groups, kw, err in (("ACGT", g, {}, TypeError), (b"ACGT", g, {}, TypeError), (["ACGT"], g, {"threshold": 1.5}, ValueError),
                                  (["ACGT"], g, {"threshold": float("nan")}, ValueError), (["ACGT"], g, {"min_af": 0.7}, ValueError),
                                  (["ACGT"], {}, {}, ValueError), (["ACGT"], {"x": ["a"], "y": ["a"]}, {}, ValueError), (["ACGT"], "x", {}, TypeError)):
        with pytest.raises(err):
            b.associate(seqs, groups, **kw)
    with pytest.raises(ValueError):
        next(b.associate_arrays(["ACGT"], g, threshold=2.0))


def test_abi_lists_the_new_entry_points():
    from bigsi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_associate.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.ASSOCIATE_SIGNATURES) == ["bigsi_hip_associate_batch", "bigsi_hip_associate_stream"]
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.ASSOCIATE_SIGNATURES[name][1] and _lib.ASSOCIATE_SIGNATURES[name][0] is C.c_int
        assert all(name not in t for t in (_lib.SIGNATURES, _lib.TALLY_SIGNATURES, _lib.CLASSIFY_SIGNATURES, _lib.WINDOW_SIGNATURES, _lib.KMERCOUNT_SIGNATURES))
        assert name not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip.h")).read(), flags=re.S)
    assert len(_lib.ASSOCIATE_SIGNATURES["bigsi_hip_associate_stream"][1]) == 11 and len(_lib.ASSOCIATE_SIGNATURES["bigsi_hip_associate_batch"][1]) == 7
    twin = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_cpu_associate.h")).read(), flags=re.S)
    assert re.findall(r"\b(bigsi_cpu_\w+)\s*\(", twin) == ["bigsi_cpu_associate"]
    assert hasattr(C.CDLL(LIB), "bigsi_cpu_associate")


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planner_and_twin(tmp_path):
    """tests/c_host/associate_sanitize_main.cpp -- a program with its own main that drives plan_associate, the group validation and the
    twin's bigsi_cpu_associate at the width edges -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of
    its own."""
    exe = str(tmp_path / "associate_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "associate_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "associate planner and twin: ok", (r.stdout[-1000:], r.stderr[-3000:])
