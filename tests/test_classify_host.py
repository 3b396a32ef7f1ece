"""Read classification without a GPU: the host planner plan_classify and the group_of validation (csrc/bigsi_launch.hpp, compiled by
g++) against a plain Python restatement (tests/classify_ref.py), the CPU twin bigsi_cpu_classify against the numpy reference on the
planted indexes the GPU tests use, the conditions those indexes must hold so that no GPU comparison passes vacuously, the host layer
(bigsi_amd/classify.py: classify_plan on collapse_plan, others, a deleted sample, the verdict rule, TSV / JSON), what BIGSI.classify
and the command line decide before any device call, and a stand-alone sanitized program over the planner and the twin."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import classify_ref as R
import tally_ref as T
from conftest import ROOT
from raw_index import ptr

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -5, -6
WIDTHS = (1, 63, 64, 65, 127, 129, 200, 775)
QUERY_COUNTS = (1, 3, 63, 64, 65)


def width_case(n_cols):
    """the planted index of a width case: 5 queries; the two widths the conditions are asserted on have the 65 of the checked layout"""
    return T.planted(n_cols, 65, seed=65) if n_cols in R.CONDITION_WIDTHS else T.planted(n_cols, 5)


# --------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("classify_host") / "libclassify_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "classify_host.cpp")])
    lib = C.CDLL(so)
    lib.classify_host_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.classify_host_bad_column.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    lib.classify_host_bad_column.restype = C.c_uint64
    return lib


def compiled_plan(lib, n_seqs, wv, n_groups):
    out = np.zeros(6, np.uint64)
    lib.classify_host_plan(n_seqs, wv, n_groups, ptr(out))
    return dict(zip(("block", "grid", "table_bytes", "lds_bytes", "too_large", "bad_groups"), (int(x) for x in out)))


def test_constants_are_the_restated_ones(plan_lib):
    c = np.zeros(3, np.uint64)
    plan_lib.classify_host_constants(ptr(c))
    assert [int(x) for x in c] == [R.BLOCK, R.MAX_GROUPS, R.NONE]
    header = open(os.path.join(ROOT, "include", "bigsi_hip_classify.h")).read()
    assert "#define BIGSI_CLASSIFY_NONE 0xFFFFFFFFu" in header and "#define BIGSI_CLASSIFY_MAX_GROUPS 4096u" in header
    from bigsi_amd import classify
    assert (classify.NONE, classify.MAX_GROUPS, classify.FIELDS) == (R.NONE, R.MAX_GROUPS, R.FIELDS) and classify.RECORD_DTYPE == R.DTYPE
    fields = re.search(r"typedef struct bigsi_hip_classify_record \{(.*?)\}", header, re.S).group(1)
    assert tuple(re.findall(r"\b([a-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))) == R.FIELDS


def test_plan_classify_against_restatement(plan_lib):
    for n_seqs in (0, 1, 2, 4095, 4096, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        for wv in (1, 4, 13, 1563, 1 << 26):
            for n_groups in (0, 1, 2, 3, 4, 5, 100, 4095, 4096, 4097, 1 << 33):
                p = compiled_plan(plan_lib, n_seqs, wv, n_groups)
                assert p == R.plan_classify(n_seqs, wv, n_groups), (n_seqs, wv, n_groups)
                assert p["grid"] == n_seqs and (p["too_large"] != 0) == (n_seqs > 0x7FFFFFFF) and p["bad_groups"] == (not 1 <= n_groups <= 4096)
                if not p["bad_groups"]:          # the table holds 12 bytes per group, the base of what follows it is 16-byte aligned, all of it within 64 KiB
                    assert n_groups * 12 <= p["table_bytes"] < n_groups * 12 + 16 and p["table_bytes"] % 16 == 0 and p["lds_bytes"] == p["table_bytes"] + 96 <= 1 << 16
    assert compiled_plan(plan_lib, 1, 1, 4096)["lds_bytes"] == 48 * 1024 + 96


def test_group_of_validation(plan_lib):
    rng = np.random.default_rng(3)
    for n, groups in ((1, 1), (200, 7), (775, 4096)):
        g = rng.integers(0, groups, n).astype(np.uint32)
        g[rng.random(n) < 0.2] = R.NONE
        assert plan_lib.classify_host_bad_column(ptr(g), n, groups) == n == R.bad_column(g, groups)
        for c in (0, n // 2, n - 1):
            bad = g.copy()
            bad[c] = groups
            assert plan_lib.classify_host_bad_column(ptr(bad), n, groups) == c == R.bad_column(bad, groups)
            bad[c] = R.NONE - 1
            assert plan_lib.classify_host_bad_column(ptr(bad), n, groups) == c
    for name in R.LAYOUTS:
        for n_cols in WIDTHS:
            g, n_groups = R.layout(name, n_cols)
            assert g.dtype == np.uint32 and g.size == n_cols and plan_lib.classify_host_bad_column(ptr(g), n_cols, n_groups) == n_cols


# --------------------------------------------------------------------------------------------- the reference's own conditions
@pytest.mark.parametrize("n_cols", R.CONDITION_WIDTHS)
def test_cases_cannot_pass_vacuously(n_cols):
    """conditions (a) .. (h), on the very planted index, layouts and thresholds the GPU width cases run"""
    p = width_case(n_cols)
    thr, i, e = p.edge_threshold()
    assert 0 < thr < 1 and T.min_kmers(int(p.us[i]), thr) == int(p.counts[i, e]) < p.us[i]
    met = R.check_conditions(p)
    assert all(met[x] for x in "abcdefgh")
    g, n_groups = R.layout("edges", n_cols)
    assert g[63] == R.NONE and g[0] == g[64 * ((n_cols - 1) // 64)] == 0 and (g == 7).sum() == 1 and g[n_cols - 1] == 7 and set(g[60:71]) == {1, R.NONE}
    g, n_groups = R.layout("spread", n_cols)
    assert [int(g[e]) for e in p.edges] == [0, 1, 2, 3, 4]


def test_records_of_is_the_definition():
    """a second, vectorised statement of the definition over the whole counts matrix"""
    p = width_case(200)
    for name in R.LAYOUTS:
        g, n_groups = R.layout(name, 200)
        for thr in R.thresholds(p) + (-0.5,):
            rec = R.records_of(p.us, p.counts, thr, g, n_groups)
            mk = np.array([T.min_kmers(int(u), thr) for u in p.us], np.int64)
            hit = (p.counts >= mk[:, None]) & (p.us > 0)[:, None] & (g != R.NONE)[None, :]
            assert np.array_equal(rec["samples_hit"], hit.sum(axis=1)) and np.array_equal(rec["num_unique"], p.us)
            assert np.array_equal(rec["min_kmers"], np.where(p.us > 0, mk, 0))
            per = np.stack([(hit & (g == x)[None, :]).sum(axis=1) for x in range(n_groups)], axis=1)
            assert np.array_equal(rec["groups_hit"], (per > 0).sum(axis=1))
            for i in np.flatnonzero(rec["groups_hit"] > 0):
                best = int(rec["best_group"][i])
                assert per[i, best] == rec["best_samples_hit"][i] and p.counts[i, rec["best_colour"][i]] == rec["best_found"][i] and hit[i, rec["best_colour"][i]]
                assert rec["best_found"][i] == np.where(hit[i], p.counts[i], -1).max()          # no hit group found more
            one = rec["groups_hit"] == 1
            assert (rec["second_group"][one] == R.NONE).all() and (rec["second_colour"][one] == R.NONE).all() and (rec["second_found"][one] == 0).all()
    assert np.array_equal(R.records_of(p.us, p.counts, -0.5, g, n_groups), R.records_of(p.us, p.counts, 0.0, g, n_groups))


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    L.bigsi_cpu_classify.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    L.bigsi_cpu_classify.restype = C.c_int32
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


def twin_classify(L, ix, seqs, thr, g, n_groups, n_entries=None):
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(seqs)
    rec = np.zeros(len(seqs) + 1, R.DTYPE)
    rec.view(np.uint8)[:] = 0xAB
    rc = L.bigsi_cpu_classify(ix, blob, ptr(off), len(seqs), T.K, thr, ptr(g), g.size if n_entries is None else n_entries, n_groups, ptr(rec))
    assert rec[-1].tobytes() == b"\xab" * 48
    return rc, rec[:-1]


def same(got, want, what):
    assert got.dtype == want.dtype == R.DTYPE
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:4], [tuple(got[i]) for i in bad[:4]], [tuple(want[i]) for i in bad[:4]])


@pytest.mark.parametrize("n_cols", WIDTHS)
def test_twin_against_numpy(cpu, n_cols):
    p = width_case(n_cols)
    sel = slice(0, 5) if n_cols not in R.CONDITION_WIDTHS else slice(None)
    ix = twin_index(cpu, p)
    for name in R.LAYOUTS:
        g, n_groups = R.layout(name, n_cols)
        for thr in R.thresholds(p):
            rc, rec = twin_classify(cpu, ix, p.seqs[sel], thr, g, n_groups)
            assert rc == 0, cpu.bigsi_cpu_last_error()
            same(rec, R.planted_records(p, thr, name)[sel], (n_cols, name, thr))
    rc, rec = twin_classify(cpu, ix, p.seqs[sel], -1.0, g, n_groups)
    same(rec, R.planted_records(p, 0.0, name)[sel], (n_cols, "a threshold below 0"))
    assert cpu.bigsi_cpu_close(ix) == 0


def test_twin_refusals(cpu):
    p = T.planted(65, 5)
    g, n_groups = R.layout("edges", 65)
    ix = twin_index(cpu, p)
    untouched = lambda rec: rec.tobytes() == b"\xab" * (48 * len(rec))
    for thr, gg, n_entries, groups in ((1.5, g, None, n_groups), (float("nan"), g, None, n_groups), (1.0, g, 64, n_groups), (1.0, g, 66, n_groups), (1.0, g, None, 0),
                                       (1.0, g, None, 4097), (1.0, g, None, 7)):          # (7 groups: the last column's id, 7, is out of range)
        rc, rec = twin_classify(cpu, ix, p.seqs, thr, gg, groups, n_entries)
        assert rc == ERR_INVALID and untouched(rec) and cpu.bigsi_cpu_last_error(), (thr, n_entries, groups)
    assert b"group_of[64]" in cpu.bigsi_cpu_last_error()
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(p.seqs)
    out = np.zeros(5, R.DTYPE)
    call = cpu.bigsi_cpu_classify
    for args in ((None, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, ptr(out)), (ix, blob, None, 5, T.K, 1.0, ptr(g), 65, n_groups, ptr(out)),
                 (ix, blob, ptr(off), 5, T.K, 1.0, None, 65, n_groups, ptr(out)), (ix, blob, ptr(off), 5, T.K, 1.0, ptr(g), 65, n_groups, None),
                 (ix, blob, ptr(off), 0, T.K, 1.0, ptr(g), 65, n_groups, ptr(out)), (ix, blob, ptr(off), 5, 0, 1.0, ptr(g), 65, n_groups, ptr(out))):
        assert call(*args) == ERR_INVALID and cpu.bigsi_cpu_last_error()
    down = off.copy()
    down[2] = down[1] - 1
    assert call(ix, blob, ptr(down), 5, T.K, 1.0, ptr(g), 65, n_groups, ptr(out)) == ERR_INVALID
    assert cpu.bigsi_cpu_close(ix) == 0
    empty = C.c_void_p()
    assert cpu.bigsi_cpu_open(C.c_uint64(64), C.c_uint64(0), C.c_uint64(8), C.c_uint32(3), 0, C.byref(empty)) == 0
    assert call(empty, blob, ptr(off), 5, T.K, 1.0, ptr(g), 0, n_groups, ptr(out)) == ERR_STATE
    assert cpu.bigsi_cpu_close(empty) == 0


# --------------------------------------------------------------------------------------------- the host layer
def test_classify_plan_on_collapse_plan():
    from bigsi_amd import classify
    from bigsi_amd.collapse import collapse_plan
    from bigsi_amd.graph.metadata import DELETION_SPECIAL_SAMPLE_NAME as GONE
    names = ["a", "b", GONE, "c", "d", "e"]
    groups = {"x": ["d", "a"], "y": ["c"]}
    g, gn = classify.classify_plan(names, groups)
    assert g.dtype == np.uint32 and g.tolist() == [0, R.NONE, R.NONE, 1, 0, R.NONE] and gn == ["x", "y"]
    want, want_names, _ = collapse_plan(names, groups)
    assert g.tolist() == want.tolist() and gn == want_names
    assert classify.classify_plan(names, [("c", "y"), ("a", "x"), ("d", "x")])[0].tolist() == [1, R.NONE, R.NONE, 0, 1, R.NONE]          # pairs: ids by first appearance
    # others: every unlisted LIVE sample in one more group; a deleted sample stays in none
    g, gn = classify.classify_plan(names, groups, others="rest")
    assert g.tolist() == [0, 2, R.NONE, 1, 0, 2] and gn == ["x", "y", "rest"]
    g, gn = classify.classify_plan(["a", "b"], {"x": ["a", "b"]}, others="rest")
    assert g.tolist() == [0, 0] and gn == ["x"]                  # nobody is left: no empty group
    # collapse_plan's refusals, unchanged
    for bad, err in (({"x": ["a"], "y": ["a"]}, ValueError), ({"x": ["a", "a"]}, ValueError), ({"x": []}, ValueError), ({}, ValueError), ({GONE: ["a"]}, ValueError),
                     ({"x": ["nobody"]}, KeyError), ({"x": [GONE]}, KeyError), ("x", TypeError), ({"x": "a"}, TypeError)):
        with pytest.raises(err):
            collapse_plan(names, bad)
        with pytest.raises(err):
            classify.classify_plan(names, bad, others="rest")
    for others, err in (("x", ValueError), (GONE, ValueError), (5, TypeError)):
        with pytest.raises(err):
            classify.classify_plan(names, groups, others=others)
    many = ["s%d" % i for i in range(4097)]
    assert len(classify.classify_plan(many, [(s, "g" + s) for s in many[:4096]])[1]) == 4096
    with pytest.raises(ValueError):
        classify.classify_plan(many, [(s, "g" + s) for s in many])
    with pytest.raises(ValueError):
        classify.classify_plan(many, [(s, "g" + s) for s in many[:4096]], others="rest")


def _records(*rows):
    rec = np.zeros(len(rows), R.DTYPE)
    for i, r in enumerate(rows):
        rec[i] = r
    return rec


def test_verdict_rule_summary_and_text():
    from bigsi_amd import classify
    N = R.NONE
    rec = _records(R.EMPTY,                                         # shorter than k
                   (40, 40, 0, 0, N, 0, N, 0, N, 0, N, 0),          # no group hit
                   (40, 19, 1, 3, 1, 25, 7, 3, N, 0, N, 0),         # one group
                   (40, 19, 2, 4, 0, 30, 2, 3, 1, 29, 9, 1),        # two groups, one k-mer apart
                   (40, 40, 2, 2, 0, 40, 2, 1, 1, 40, 9, 1),        # two groups hold the read whole
                   (40, 19, 3, 5, 1, 30, 9, 2, 0, 28, 2, 2))        # two k-mers apart
    gn = ["human", "mouse"]
    assert classify.verdicts(rec, gn) == [("skipped", None), ("unclassified", None), ("assigned", "mouse"), ("assigned", "human"), ("ambiguous", None), ("assigned", "mouse")]
    assert classify.verdicts(rec, gn, margin=2) == [("skipped", None), ("unclassified", None), ("assigned", "mouse"), ("ambiguous", None), ("ambiguous", None), ("assigned", "mouse")]
    assert classify.verdicts(rec, gn, margin=3)[5] == ("ambiguous", None) and classify.verdicts(rec, gn, margin=0)[4] == ("assigned", "human")
    for bad, err in ((-1, ValueError), (True, TypeError), (1.0, TypeError), ("1", TypeError)):
        with pytest.raises(err):
            classify.verdicts(rec, gn, margin=bad)
    names = {2: "s2", 7: 'se\tven', 9: None}
    res = classify.result(rec, gn, names.get)
    assert list(res) == ["groups", "records", "summary"] and res["groups"] == gn
    assert res["summary"] == {"reads": 6, "assigned": {"human": 1, "mouse": 2}, "ambiguous": 1, "unclassified": 1, "skipped": 1}
    assert res["records"][3] == {"verdict": "assigned", "group": "human", "best_sample": "s2", "num_kmers": 40, "min_kmers": 19, "groups_hit": 2, "samples_hit": 4,
                                 "best_group": "human", "best_found": 30, "best_colour": 2, "best_samples_hit": 3, "second_group": "mouse", "second_found": 29,
                                 "second_colour": 9, "second_samples_hit": 1}
    assert res["records"][0]["best_group"] is None and res["records"][0]["best_colour"] is None and res["records"][0]["best_sample"] is None
    assert res["records"][5]["best_sample"] is None and res["records"][5]["best_colour"] == 9          # a colour without a name: the colour alone
    assert all(type(v) is int for r in res["records"] for k_, v in r.items() if k_.endswith(("found", "hit", "kmers")))
    assert classify.result(rec, gn, names.get, margin=2)["summary"]["assigned"] == {"human": 0, "mouse": 2}
    ids = ["r%d" % i for i in range(6)]
    assert json.loads(classify.to_json(res, ids)) == {"groups": gn, "records": [dict({"name": n}, **r) for n, r in zip(ids, res["records"])], "summary": res["summary"]}
    assert json.loads(classify.to_json(res, ids, summary_only=True)) == {"groups": gn, "summary": res["summary"]} and json.loads(classify.to_json(res))["records"] == res["records"]
    tail = "# reads\t6\n# assigned human\t1\n# assigned mouse\t2\n# ambiguous\t1\n# unclassified\t1\n# skipped\t1"
    assert classify.to_tsv(res, ids) == ("name\tverdict\tgroup\tbest_found\tnum_kmers\tsecond_group\tsecond_found\tbest_sample\n"
                                        "r0\tskipped\t\t0\t0\t\t0\t\n"
                                        "r1\tunclassified\t\t0\t40\t\t0\t\n"
                                        "r2\tassigned\tmouse\t25\t40\t\t0\tse ven\n"
                                        "r3\tassigned\thuman\t30\t40\tmouse\t29\ts2\n"
                                        "r4\tambiguous\t\t40\t40\tmouse\t40\ts2\n"
                                        "r5\tassigned\tmouse\t30\t40\thuman\t28\t\n" + tail)
    assert classify.to_tsv(res, ids, summary_only=True) == tail
    assert classify.result(np.zeros(0, R.DTYPE), gn, names.get) == {"groups": gn, "records": [], "summary": {"reads": 0, "assigned": {"human": 0, "mouse": 0}, "ambiguous": 0,
                                                                                                          "unclassified": 0, "skipped": 0}}


class _FakeIndex(object):
    def __init__(self):
        self.asked = None

    def classify(self, seqs, groups, threshold=1.0, margin=1, others=None):
        from bigsi_amd import classify
        self.asked = (list(seqs), list(groups), threshold, margin, others)
        return classify.result(_records((9, 9, 1, 1, 0, 9, 4, 1, R.NONE, 0, R.NONE, 0), R.EMPTY), ["g"], {4: "s4"}.get, margin)


def test_cli_parsing_text_and_refusals(tmp_path, capsys):
    from bigsi_amd.__main__ import build_parser, classify_text, main
    p = build_parser()[0]
    a = p.parse_args(["classify", "reads.fasta", "--groups", "g.tsv", "-c", "c.yaml"])
    assert (a.cmd, a.fasta, a.groups, a.threshold, a.margin, a.others, a.format, a.summary_only, a.config) == ("classify", "reads.fasta", "g.tsv", 1.0, 1, None, "tsv", False, "c.yaml")
    a = p.parse_args(["classify", "r.fa", "--groups", "g.tsv", "-t", "0.4", "--margin", "3", "--others", "rest", "--format", "json", "--summary-only"])
    assert (a.threshold, a.margin, a.others, a.format, a.summary_only) == (0.4, 3, "rest", "json", True)
    for argv in (["classify"], ["classify", "r.fa"], ["classify", "r.fa", "--groups", "g", "--margin", "-1"], ["classify", "r.fa", "--groups", "g", "--format", "csv"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    p.format_help()
    ix = _FakeIndex()
    text = classify_text(ix, [("q0", "ACGT"), ("q1", "TT")], [("s4", "g")], 0.5, 2, "rest")
    assert ix.asked == (["ACGT", "TT"], [("s4", "g")], 0.5, 2, "rest")
    assert text.split("\n")[:3] == ["name\tverdict\tgroup\tbest_found\tnum_kmers\tsecond_group\tsecond_found\tbest_sample", "q0\tassigned\tg\t9\t9\t\t0\ts4", "q1\tskipped\t\t0\t0\t\t0\t"]
    assert json.loads(classify_text(ix, [("q0", "ACGT"), ("q1", "TT")], [("s4", "g")], fmt="json"))["records"][0]["name"] == "q0"
    assert classify_text(ix, [("q0", "A"), ("q1", "T")], [("s4", "g")], summary_only=True) == "# reads\t2\n# assigned g\t1\n# ambiguous\t0\n# unclassified\t0\n# skipped\t1"
    # refused before any device call: --sharded, a threshold above 1, a groups file that cannot be read or names a sample twice
    good, twice = tmp_path / "g.tsv", tmp_path / "twice.tsv"
    good.write_text("s0\tx\ns1\ty\n")
    twice.write_text("s0\tx\ns0\ty\n")
    for argv, words in ((["classify", "r.fa", "--groups", str(good), "--sharded"], ("--sharded", "classify")), (["classify", "r.fa", "--groups", str(good), "-t", "1.5"], ("threshold",)),
                        (["classify", "r.fa", "--groups", str(tmp_path / "missing.tsv")], ("--groups",)), (["classify", "r.fa", "--groups", str(twice)], ("two groups",))):
        with pytest.raises(SystemExit):
            main(argv)
        err = capsys.readouterr().err
        assert all(w in err for w in words), (argv, err)


def test_classify_checks_its_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    g = {"x": ["a"]}
    for seqs, groups, kw, err in (("ACGT", g, {}, TypeError), (b"ACGT", g, {}, TypeError), (["ACGT"], g, {"threshold": 1.5}, ValueError),
                                  (["ACGT"], g, {"threshold": float("nan")}, ValueError), (["ACGT"], g, {"margin": -1}, ValueError), (["ACGT"], g, {"margin": 1.5}, TypeError),
                                  (["ACGT"], {}, {}, ValueError), (["ACGT"], {"x": ["a"], "y": ["a"]}, {}, ValueError), (["ACGT"], "x", {}, TypeError)):
        with pytest.raises(err):
            b.classify(seqs, groups, **kw)
    with pytest.raises(ValueError):
        next(b.classify_arrays(["ACGT"], g, threshold=2.0))


def test_abi_lists_the_new_entry_points():
    from bigsi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_classify.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.CLASSIFY_SIGNATURES) == ["bigsi_hip_classify_batch", "bigsi_hip_classify_stream"]
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.CLASSIFY_SIGNATURES[name][1] and _lib.CLASSIFY_SIGNATURES[name][0] is C.c_int
        assert all(name not in t for t in (_lib.SIGNATURES, _lib.TALLY_SIGNATURES, _lib.WINDOW_SIGNATURES, _lib.KMERCOUNT_SIGNATURES))
        assert name not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip.h")).read(), flags=re.S)
    assert len(_lib.CLASSIFY_SIGNATURES["bigsi_hip_classify_stream"][1]) == 10 and len(_lib.CLASSIFY_SIGNATURES["bigsi_hip_classify_batch"][1]) == 6
    assert "bigsi_cpu_classify" in open(os.path.join(ROOT, "include", "bigsi_cpu_classify.h")).read()


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planner_and_twin(tmp_path):
    """tests/c_host/classify_sanitize_main.cpp -- a program with its own main that drives plan_classify, classify_bad_column and the
    twin's bigsi_cpu_classify over odd shapes -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its
    own."""
    exe = str(tmp_path / "classify_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "classify_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "classify planner and twin: ok", (r.stdout[-1000:], r.stderr[-3000:])
