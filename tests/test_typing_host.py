"""Locus typing without a GPU: the conditions the planted cases must hold so that no GPU comparison passes vacuously, the host planner
plan_typing, the key function typing_key -- the one function k_locus_best compiles -- and the label validation
(csrc/bigsi_launch.hpp, compiled by g++) against a plain Python restatement (tests/typing_ref.py) and Python integers, the CPU twin
bigsi_cpu_typing against the numpy reference on the planted indexes the GPU tests use, the host layer (bigsi_amd/locus_typing.py:
parse_scheme, slices, calls, parse_profiles, assign_st, result, TSV / JSON), what BIGSI.typing_arrays and the command line decide
before any device call, the ABI lists, and a stand-alone sanitized program over the planner, the key and the twin."""
import ctypes as C
import json
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import tally_ref as T
import typing_ref as R
from conftest import ROOT
from raw_index import ptr

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_NOMEM, ERR_CAPACITY, ERR_STATE = -1, -3, -5, -6
PLAN_FIELDS = ("block", "tile", "word_groups", "tiles", "grid", "loci_grid", "words_grid", "counts_grid", "cell_bytes", "too_large", "bad_loci", "too_many_bytes")


# --------------------------------------------------------------------------------------------- outputs with guards
class Out(object):
    """The five outputs of a fetch, preset to 0xAB, with a guard row behind each"""

    def __init__(self, n_loci, n_cols):
        self.nl, self.n_cols = n_loci, n_cols
        self.best, self.hits = np.zeros((n_loci + 1, n_cols), np.uint64), np.zeros((n_loci + 1, n_cols), np.uint32)
        self.loci, self.samples, self.records = np.zeros((n_loci + 1, 3), np.uint32), np.zeros((n_cols + 1, 2), np.uint32), np.zeros(n_loci + 1, np.uint32)
        for a in self.arrays():
            a.view(np.uint8)[:] = 0xAB

    def arrays(self):
        return (self.best, self.hits, self.loci, self.samples, self.records)

    def guards_hold(self):
        return all(a[-1].tobytes() == b"\xab" * a[-1].nbytes for a in self.arrays())

    def untouched(self):
        return all(a.tobytes() == b"\xab" * a.nbytes for a in self.arrays())

    def got(self, cells=True):
        assert self.guards_hold()
        return dict(best=self.best[:-1] if cells else None, hits=self.hits[:-1] if cells else None, loci=self.loci[:-1], samples=self.samples[:-1],
                    records=self.records[:-1])


def same(got, want, what):
    """the outputs of a fetch against the reference, bit for bit"""
    for key in ("loci", "samples", "records", "best", "hits"):
        if got[key] is None:
            continue
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
        bad = np.argwhere(got[key] != want[key])
        assert bad.size == 0, (what, key, bad[:4].tolist(), [hex(int(got[key][tuple(i)])) for i in bad[:4]], [hex(int(want[key][tuple(i)])) for i in bad[:4]])


# --------------------------------------------------------------------------------------------- the reference's own conditions
@pytest.mark.parametrize("n_cols", R.CONDITION_WIDTHS)
def test_cases_cannot_pass_vacuously(n_cols):
    """on the very planted indexes, layouts and thresholds the GPU cases run: a cell whose winner is not the lowest identity among
    its hits, a tie resolved to the lowest identity, a winner with a partial score, a cell with hits >= 2, an empty cell, a locus
    without records, a locus whose records lie in different tiles"""
    p = R.width_case(n_cols)
    thr, i, e = p.edge_threshold()
    assert 0 < thr < 1 and T.min_kmers(int(p.us[i]), thr) == int(p.counts[i, e]) < p.us[i] and R.thresholds(p) == (1.0, 0.4, thr, 0.0)
    seen = {}
    for x in R.thresholds(p):
        seen[x] = R.check_conditions(p, x)
        print(n_cols, x, {k: (len(v) if k == "scores" else v) for k, v in seen[x].items()})
    assert seen[0.4]["called"] > seen[1.0]["called"] and seen[0.0]["called"] == R.LOCI_WITH_RECORDS * n_cols          # at 0 every column hits, with c = 0 in most
    assert 0 in seen[0.0]["scores"] and R.EXACT in seen[0.0]["scores"]
    assert R.two_tile_locus("interleaved", R.N_QUERIES) == (16, 32, 64) and R.two_tile_locus("grouped", R.N_QUERIES) == (23, 63, 64)
    assert (-(-n_cols // 64)) % 2 == (0 if n_cols == 200 else 1)          # 775 columns: an odd number of result words, a pad word behind them


def test_scheme_and_layouts():
    locus, allele, nl = R.labels(R.N_QUERIES)
    assert nl == R.N_LOCI == 26 and locus.max() == 23 and allele.tolist() == list(range(64, -1, -1))
    assert locus[:6].tolist() == [0, 0, 1, 1, 2, 2] and locus[46:50].tolist() == [23, 23, 0, 1] and locus[64] == 16
    for name in R.LAYOUTS:
        order, lo, al, n = R.layout(name, R.N_QUERIES)
        assert sorted(order.tolist()) == list(range(R.N_QUERIES)) and n == nl and np.array_equal(al, allele[order])
        keep = lo != R.NONE
        assert np.array_equal(lo[keep], locus[order][keep]) and ((~keep).sum() > 0) == (name == "shuffled")
    assert (np.diff(R.layout("grouped", R.N_QUERIES)[1].astype(np.int64)) >= 0).all()
    assert not (np.diff(R.layout("interleaved", R.N_QUERIES)[1].astype(np.int64)) >= 0).all()


def test_typing_of_is_the_definition():
    """a second statement of the definition, in exact fractions: the winner of a cell is the record with the highest c / u among the
    locus's records that hit the column, the lowest identity among equals -- all u here are far below 2^16, so scores and fractions
    order alike"""
    from bigsi_amd import locus_typing
    p = R.width_case(200)
    assert int(p.us.max()) ** 2 < 1 << 32
    columns, drop = R.column_mask(p)
    for thr in R.thresholds(p) + (-0.5,):
        hit = R.hits_of(p, thr)
        for name in R.LAYOUTS:
            for masked in (False, True):
                order, lo, al, nl = R.layout(name, len(p.seqs))
                g = R.typing_of(p.us, p.counts, hit, order, lo, al, nl, columns if masked else None)
                allele, score, exact = locus_typing.decode(g["best"])
                for l in range(nl):
                    pos = [i for i in range(len(order)) if lo[i] == l and p.us[order[i]] > 0]
                    assert g["records"][l] == len(pos)
                    for s in range(200):
                        mine = [(Fraction(int(p.counts[order[i], s]), int(p.us[order[i]])), -int(al[i])) for i in pos if hit[order[i], s] and not (masked and s == drop)]
                        assert g["hits"][l, s] == len(mine)
                        if not mine:
                            assert g["best"][l, s] == 0 and allele[l, s] == -1 and not exact[l, s]
                            continue
                        frac, neg = max(mine)
                        assert allele[l, s] == -neg and int(score[l, s]) == int(frac * R.EXACT) and exact[l, s] == (frac == 1), (thr, name, masked, l, s)
                assert g["loci"][:, 0].tolist() == (allele >= 0).sum(axis=1).tolist() and g["loci"][:, 1].tolist() == exact.sum(axis=1).tolist()
                assert g["loci"][:, 2].tolist() == (g["hits"] > 1).sum(axis=1).tolist()
                assert g["samples"][:, 0].tolist() == (allele >= 0).sum(axis=0).tolist() and g["samples"][:, 1].tolist() == exact.sum(axis=0).tolist()
    a, b = R.typing_of(p.us, p.counts, R.hits_of(p, -0.5), order, lo, al, nl), R.typing_of(p.us, p.counts, R.hits_of(p, 0.0), order, lo, al, nl)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # a record added twice counts twice in hits and records and changes nothing in best
    twice = R.typing_of(p.us, p.counts, R.hits_of(p, 0.4), np.tile(order, 2), np.tile(lo, 2), np.tile(al, 2), nl)
    once = R.typing_of(p.us, p.counts, R.hits_of(p, 0.4), order, lo, al, nl)
    assert np.array_equal(twice["best"], once["best"]) and np.array_equal(twice["hits"], 2 * once["hits"]) and np.array_equal(twice["records"], 2 * once["records"])


# --------------------------------------------------------------------------------------------- the planner and the key
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("typing_host") / "libtyping_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "typing_host.cpp")])
    lib = C.CDLL(so)
    lib.typing_host_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.typing_host_key.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.typing_host_key.restype = C.c_uint64
    lib.typing_host_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.typing_host_bad_label.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
    lib.typing_host_bad_label.restype = C.c_uint64
    return lib


def compiled_plan(lib, n_seqs, wv, n_loci):
    out = np.zeros(len(PLAN_FIELDS), np.uint64)
    lib.typing_host_plan(n_seqs, wv, n_loci, ptr(out))
    return dict(zip(PLAN_FIELDS, (int(x) for x in out)))


def test_constants_are_the_restated_ones(plan_lib):
    c = np.zeros(8, np.uint64)
    plan_lib.typing_host_constants(ptr(c))
    assert [int(x) for x in c] == [R.BLOCK, R.NONE, R.MAX_ALLELE, R.MAX_LOCI, R.CELL_BYTES, R.TILE, R.LOADS, T.CHUNK_SEQS]
    assert R.TILE <= R.BLOCK and R.TILE % R.LOADS == 0
    header = open(os.path.join(ROOT, "include", "bigsi_hip_typing.h")).read()
    assert "#define BIGSI_TYPING_NONE 0xFFFFFFFFu" in header and "#define BIGSI_TYPING_MAX_LOCI (1u << 20)" in header
    assert "#define BIGSI_TYPING_MAX_ALLELE 0xFFFFFFFEu" in header and "#define BIGSI_TYPING_CELL_BYTES (4ull << 30)" in header
    assert "DESIGN limit, not a\n * measured one" in header and "u_i * u_j > 2^32" in header and "added twice counts twice" in header
    from bigsi_amd import locus_typing
    assert (locus_typing.NONE, locus_typing.MAX_ALLELE, locus_typing.MAX_LOCI, locus_typing.EXACT_SCORE) == (R.NONE, R.MAX_ALLELE, R.MAX_LOCI, R.EXACT)


def test_plan_typing_against_restatement(plan_lib):
    for n_seqs in (0, 1, 63, 64, 65, 128, 129, 4096, 64 * 0x7FFFFFFF, 64 * 0x7FFFFFFF + 1, 1 << 40):
        for wv in (1, 2, 3, 4, 5, 13, 1563, 15625, 4 * 0x7FFFFFFF, 4 * 0x7FFFFFFF + 1, 1 << 34, 1 << 62, (1 << 64) - 1):
            for n_loci in (0, 1, 2, 3, 4, 5, 63, 64, 65, 357, 358, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 40):
                p = compiled_plan(plan_lib, n_seqs, wv, n_loci)
                assert p == R.plan_typing(n_seqs, wv, n_loci), (n_seqs, wv, n_loci)
                assert p["grid"] == min(-(-wv // 4) * -(-n_seqs // 64), (1 << 64) - 1) and p["bad_loci"] == (not 1 <= n_loci <= 1 << 20)
                if not p["bad_loci"]:
                    assert p["too_many_bytes"] == (768 * n_loci * wv > 4 << 30) and p["loci_grid"] == -(-n_loci // 4)
                    assert p["cell_bytes"] == (0 if p["too_many_bytes"] else 768 * n_loci * wv) and p["counts_grid"] == p["loci_grid"] + p["words_grid"]
    # grids above 2^31 - 1 are refused; the last one that is not
    assert compiled_plan(plan_lib, 64 * 0x7FFFFFFF, 1, 1)["too_large"] == 0 and compiled_plan(plan_lib, 64 * 0x7FFFFFFF + 1, 1, 1)["too_large"] == 0x80000000
    assert compiled_plan(plan_lib, 1, 4 * 0x7FFFFFFF - 4, 1)["too_large"] == 0 and compiled_plan(plan_lib, 1, 4 * 0x7FFFFFFF, 1)["too_large"] == 0x80000000          # (the count launch: + 1 for the locus)
    assert compiled_plan(plan_lib, 1, 4 * 0x7FFFFFFF, 0)["too_large"] == 0 and compiled_plan(plan_lib, 1, 4 * 0x7FFFFFFF + 1, 0)["too_large"] == 0x80000000
    assert compiled_plan(plan_lib, 65 * 64, 1 << 33, 1)["too_large"] == 65 << 31 and compiled_plan(plan_lib, 1 << 40, 1 << 62, 1)["too_large"] == (1 << 64) - 1          # (saturated)
    # the 4 GiB design limit: 12 bytes per cell, rows of whole words -- a million samples (15625 words) take 357 loci, not 358
    assert compiled_plan(plan_lib, 1, 15625, 357)["too_many_bytes"] == 0 and compiled_plan(plan_lib, 1, 15625, 358)["too_many_bytes"] == 1
    assert compiled_plan(plan_lib, 1, 5, 1 << 20)["cell_bytes"] == 5 * 768 << 20 and compiled_plan(plan_lib, 1, 6, 1 << 20)["too_many_bytes"] == 1
    assert compiled_plan(plan_lib, 1, 1 << 62, 1 << 20) == R.plan_typing(1, 1 << 62, 1 << 20)          # (the product does not fit 64 bits)


def test_key_against_python_integers(plan_lib):
    key = plan_lib.typing_host_key
    for u in (1, 2, 65535, 65536, 1 << 20, (1 << 32) - 1):
        for c in sorted({0, 1, u - 1, u}):
            if c > u:
                continue
            for allele in (0, 1, 12345, 0xFFFFFFFE):
                got = key(c, u, allele)
                assert got == R.key_of(c, u, allele) == (c * 0xFFFFFFFF // u) << 32 | (0xFFFFFFFF - allele), (c, u, allele)
                assert got != 0 and (got >> 32 == 0xFFFFFFFF) == (c == u) and 0xFFFFFFFF - (got & 0xFFFFFFFF) == allele
    rng = np.random.default_rng(5)
    u = np.maximum(rng.integers(1, 1 << 32, 200000, dtype=np.uint64) >> rng.integers(0, 32, 200000, dtype=np.uint64), 1).astype(np.uint32)
    c = (rng.integers(0, 1 << 32, 200000, dtype=np.uint64) % (u.astype(np.uint64) + 1)).astype(np.uint32)
    allele = rng.integers(0, 0xFFFFFFFF, 200000, dtype=np.uint64).astype(np.uint32)
    out = np.zeros(200000, np.uint64)
    plan_lib.typing_host_keys(ptr(c), ptr(u), ptr(allele), 200000, ptr(out))
    assert (u >= 1 << 31).any() and (u < 256).any() and (c == u).any()
    assert out.tolist() == [R.key_of(x, y, z) for x, y, z in zip(c.tolist(), u.tolist(), allele.tolist())]
    from bigsi_amd import locus_typing
    assert locus_typing.key_of(3, 7, 9) == key(3, 7, 9)


def test_key_is_monotone_in_the_fraction(plan_lib):
    """over all u <= 64: a higher c / u is a higher key whatever the identities, and equal fractions order by identity, lowest first"""
    pairs = [(c, u) for u in range(1, 65) for c in range(u + 1)]
    keyed = sorted((Fraction(c, u), plan_lib.typing_host_key(c, u, 0xFFFFFFFE) >> 32, plan_lib.typing_host_key(c, u, 0) >> 32) for c, u in pairs)
    for (f1, lo1, hi1), (f2, lo2, hi2) in zip(keyed, keyed[1:]):
        assert lo1 == hi1 and lo2 == hi2
        assert (lo1 == lo2) if f1 == f2 else (lo1 < lo2), (f1, f2)
    key = plan_lib.typing_host_key
    assert key(2, 3, 0xFFFFFFFE) > key(1, 2, 0) and key(1, 2, 7) > key(2, 4, 8) > key(32, 64, 9) and key(0, 5, 3) > key(0, 9, 4) > 0


def test_label_validation(plan_lib):
    lo, al = np.array([0, 1, 5, R.NONE, 4], np.uint32), np.array([7, 7, 7, 0xFFFFFFFF, 7], np.uint32)
    bad = plan_lib.typing_host_bad_label
    assert bad(ptr(lo), ptr(al), 5, 6) == 5 and bad(ptr(lo), ptr(al), 5, 5) == 2 and bad(ptr(lo), ptr(al), 2, 2) == 2 and bad(ptr(lo), ptr(al), 5, 1) == 1
    assert bad(ptr(lo), ptr(al), 0, 1) == 0
    al[4] = 0xFFFFFFFF
    assert bad(ptr(lo), ptr(al), 5, 6) == 4
    al[4] = 0xFFFFFFFE
    lo[2] = 0xFFFFFFFE
    assert bad(ptr(lo), ptr(al), 5, 1 << 20) == 2 and bad(ptr(lo), ptr(al), 5, 1 << 32) == 5


# --------------------------------------------------------------------------------------------- the CPU twin
TWIN_ARGS = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
             C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]


@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    L.bigsi_cpu_typing.argtypes = TWIN_ARGS
    L.bigsi_cpu_typing.restype = C.c_int32
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


def twin_typing(L, ix, n_cols, seqs, thr, locus_of, allele_of, n_loci, columns=None, cells=True, cell_cap=None, sample_cap=None):
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(seqs)
    out = Out(min(max(n_loci, 1), 64), n_cols)
    locus_of, allele_of = np.ascontiguousarray(locus_of, np.uint32), np.ascontiguousarray(allele_of, np.uint32)
    rc = L.bigsi_cpu_typing(ix, blob, ptr(off), len(seqs), T.K, thr, ptr(locus_of), ptr(allele_of), n_loci, ptr(columns), ptr(out.best) if cells else None,
                            ptr(out.hits) if cells else None, out.nl * n_cols if cell_cap is None else cell_cap, ptr(out.loci), ptr(out.samples),
                            n_cols if sample_cap is None else sample_cap, ptr(out.records))
    assert out.guards_hold()
    return rc, out


@pytest.mark.parametrize("n_cols", R.WIDTHS)
def test_twin_against_numpy(cpu, n_cols):
    p = R.width_case(n_cols)
    ix = twin_index(cpu, p)
    columns = R.column_mask(p)[0]
    for name in R.LAYOUTS:
        order, lo, al, nl = R.layout(name, len(p.seqs))
        seqs = [p.seqs[q] for q in order]
        for thr in R.thresholds(p):
            for masked in (False, True):
                rc, out = twin_typing(cpu, ix, n_cols, seqs, thr, lo, al, nl, columns if masked else None)
                assert rc == 0, cpu.bigsi_cpu_last_error()
                same(out.got(), R.planted_typing(p, thr, name, masked), (n_cols, name, thr, masked))
    rc, out = twin_typing(cpu, ix, n_cols, seqs, -1.0, lo, al, nl, cells=False)
    assert rc == 0 and out.best.tobytes() == b"\xab" * out.best.nbytes and out.hits.tobytes() == b"\xab" * out.hits.nbytes
    same(out.got(cells=False), R.planted_typing(p, 0.0, name), (n_cols, "a threshold below 0, no cells"))
    assert cpu.bigsi_cpu_close(ix) == 0


def test_twin_refusals(cpu):
    p = R.width_case(65)
    order, lo, al, nl = R.layout("grouped", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    ix = twin_index(cpu, p)
    bad_locus, bad_allele, none_allele = lo.copy(), al.copy(), al.copy()
    bad_locus[7] = nl
    bad_allele[9] = 0xFFFFFFFF
    for kw, rc_want, word in ((dict(thr=1.5), ERR_INVALID, b"threshold"), (dict(thr=float("nan")), ERR_INVALID, b"threshold"), (dict(n_loci=0), ERR_INVALID, b"BIGSI_TYPING_MAX_LOCI"),
                              (dict(n_loci=(1 << 20) + 1), ERR_INVALID, b"BIGSI_TYPING_MAX_LOCI"), (dict(locus_of=bad_locus), ERR_INVALID, b"locus_of[7]"),
                              (dict(allele_of=bad_allele), ERR_INVALID, b"allele_of[9]"), (dict(n_loci=23), ERR_INVALID, b"locus_of["),
                              (dict(cell_cap=nl * 65 - 1), ERR_CAPACITY, b"cell"), (dict(sample_cap=64), ERR_CAPACITY, b"sample_counts")):
        args = dict(thr=1.0, locus_of=lo, allele_of=al, n_loci=nl)
        args.update(kw)
        rc, out = twin_typing(cpu, ix, 65, seqs, args["thr"], args["locus_of"], args["allele_of"], args["n_loci"], cell_cap=args.get("cell_cap"), sample_cap=args.get("sample_cap"))
        assert rc == rc_want and out.untouched() and word in cpu.bigsi_cpu_last_error(), (kw, cpu.bigsi_cpu_last_error())
    # the identity of a record without a locus is not looked at
    no_locus = lo.copy()
    no_locus[9] = R.NONE
    rc, out = twin_typing(cpu, ix, 65, seqs, 1.0, no_locus, bad_allele, nl)
    assert rc == 0, cpu.bigsi_cpu_last_error()
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(seqs)
    out = Out(nl, 65)
    call = cpu.bigsi_cpu_typing
    tail = (ptr(out.best), ptr(out.hits), nl * 65, ptr(out.loci), ptr(out.samples), 65, ptr(out.records))
    head = (blob, ptr(off), len(seqs), T.K, 1.0, ptr(lo), ptr(al), nl, None)
    for args in ((None,) + head + tail, (ix, blob, None) + head[2:] + tail, (ix,) + head[:5] + (None,) + head[6:] + tail, (ix,) + head[:6] + (None,) + head[7:] + tail,
                 (ix,) + head + tail[:3] + (None,) + tail[4:], (ix,) + head + tail[:4] + (None,) + tail[5:], (ix,) + head + tail[:6] + (None,),
                 (ix, blob, ptr(off), 0) + head[3:] + tail, (ix, blob, ptr(off), len(seqs), 0) + head[4:] + tail):
        assert call(*args) == ERR_INVALID and cpu.bigsi_cpu_last_error()
    down = off.copy()
    down[2] = down[1] - 1
    assert call(ix, blob, ptr(down), *head[2:], *tail) == ERR_INVALID and out.untouched()
    assert cpu.bigsi_cpu_close(ix) == 0
    empty = C.c_void_p()
    assert cpu.bigsi_cpu_open(C.c_uint64(64), C.c_uint64(0), C.c_uint64(8), C.c_uint32(3), 0, C.byref(empty)) == 0
    assert call(empty, *head, *tail) == ERR_STATE and out.untouched()
    assert cpu.bigsi_cpu_close(empty) == 0


# --------------------------------------------------------------------------------------------- the host layer
SCHEME = ">adk_1 first\nAAAA\n>fumC_7\nCCCC\n>adk_2\nGG\nGG\n>arcA_new_3\nTTTT\n>fumC_12\nACGT\n>blaCTX-M-15\nTTAA\n"
LOCI_MAP = "blaCTX-M-15\tblaCTX-M\n# a comment\n\nadk_2\tadk\n"


def test_parse_scheme(tmp_path):
    from bigsi_amd import locus_typing as lt
    for scheme in (SCHEME, SCHEME.encode()):
        loci, names, alleles, records, locus_of, allele_of = lt.parse_scheme(scheme, LOCI_MAP)
        assert loci == ["adk", "fumC", "arcA_new", "blaCTX-M"]                                        # order of first appearance; split at the LAST _
        assert names == ["adk_1", "fumC_7", "adk_2", "arcA_new_3", "fumC_12", "blaCTX-M-15"] and alleles == ["1", "7", "2", "3", "12", "blaCTX-M-15"]
        assert records == ["AAAA", "GGGG", "CCCC", "ACGT", "TTTT", "TTAA"] and locus_of.tolist() == [0, 0, 1, 1, 2, 3] and allele_of.tolist() == [0, 2, 1, 4, 3, 5]
        assert locus_of.dtype == allele_of.dtype == np.uint32
    f, m = tmp_path / "scheme.fa", tmp_path / "map.tsv"
    f.write_text(SCHEME)
    m.write_text(LOCI_MAP)
    assert lt.parse_scheme(str(f), str(m))[0] == loci and lt.parse_scheme(str(f), {"blaCTX-M-15": "bla", "adk_1": "x"})[0] == ["x", "fumC", "adk", "arcA_new", "bla"]
    assert lt.parse_scheme("")[0] == [] and lt.parse_scheme("")[4].size == 0
    with pytest.raises(ValueError, match="no locus"):
        lt.parse_scheme(SCHEME)                                                                      # blaCTX-M-15 has no _ and no map
    with pytest.raises(ValueError, match="twice"):
        lt.parse_scheme(">adk_1\nAAAA\n>adk_1\nCCCC\n")
    for bad in (">_1\nAAAA\n", ">adk_\nAAAA\n"):
        with pytest.raises(ValueError, match="no locus"):
            lt.parse_scheme(bad)
    for bad, word in (("adk_1\n", "expected"), ("adk_1\tadk\textra\n", "expected"), ("adk_1\tadk\nadk_1\tfumC\n", "two loci")):
        with pytest.raises(ValueError, match=word):
            lt.parse_loci_map(bad)


def test_slices():
    from bigsi_amd import locus_typing as lt
    lo = np.array([0, 0, 1, R.NONE, 2, 4, 4], np.uint32)
    one = lt.slices(lo, 5, 65, 1 << 30)
    assert len(one) == 1 and one[0][:2] == (0, 5) and one[0][2].tolist() == [0, 1, 2, 4, 5, 6] and one[0][3].tolist() == [0, 0, 1, 2, 4, 4]
    # 65 columns are two words: 128 cells of 12 bytes per locus; 3072 bytes hold two loci
    got = lt.slices(lo, 5, 65, 3072)
    assert [(a, b, i.tolist(), r.tolist()) for a, b, i, r in got] == [(0, 2, [0, 1, 2], [0, 0, 1]), (2, 4, [4], [0]), (4, 5, [5, 6], [0, 0])]
    assert [(a, b) for a, b, _, _ in lt.slices(lo, 5, 65, 1)] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]          # at least one locus each
    assert len(lt.slices(lo, 5, 64, 1536)) == 3 and len(lt.slices(lo, 5, 64, 1535)) == 5


def _case():
    """three loci (adk, fumC, gyrB) over five columns, column 3 deleted: cells and counts as the device would leave them"""
    from bigsi_amd import locus_typing as lt
    k = lt.key_of
    best = np.array([[k(9, 9, 0), k(9, 9, 1), k(4, 9, 1), 0, k(9, 9, 0)],
                     [k(5, 5, 3), k(5, 5, 2), k(5, 5, 2), 0, k(5, 5, 3)],
                     [k(7, 7, 4), k(7, 7, 5), 0, 0, k(7, 7, 5)]], np.uint64)
    hits = np.array([[1, 2, 1, 0, 1], [1, 1, 3, 0, 1], [1, 1, 0, 0, 1]], np.uint32)
    lc = np.array([[4, 3, 1], [4, 4, 1], [3, 3, 0]], np.uint32)
    sc = np.array([[3, 3], [3, 3], [2, 1], [0, 0], [3, 3]], np.uint32)
    return best, hits, lc, sc, np.array([2, 2, 2], np.uint32)


ALLELES = ["1", "2", "7", "12", "3", "4"]          # by identity
PROFILES = "ST\tadk\tclonal_complex\tgyrB\tfumC\n10\t1\tCC10\t3\t12\n11\t2\tCC10\t4\t7\n12\t1\tCC10\t3\t12\n"


def test_calls_profiles_result_and_text():
    from bigsi_amd import locus_typing as lt
    best, hits, lc, sc, rec = _case()
    allele, score, exact = lt.decode(best)
    assert allele.tolist() == [[0, 1, 1, -1, 0], [3, 2, 2, -1, 3], [4, 5, -1, -1, 5]] and exact[0].tolist() == [True, True, False, False, True]
    assert score[0, 2] == 4 * 0xFFFFFFFF // 9
    m = lt.calls(best, ALLELES, hits)
    assert m[0][0] == {"allele": "1", "fraction": 1.0, "exact": True, "n_hits": 1} and m[0][3] is None and m[2][2] is None
    assert m[0][2] == {"allele": "2", "fraction": (4 * 0xFFFFFFFF // 9) / 0xFFFFFFFF, "exact": False, "n_hits": 1} and m[1][2]["n_hits"] == 3
    assert "n_hits" not in lt.calls(best, ALLELES)[0][0]
    loci = ["adk", "fumC", "gyrB"]
    table = lt.parse_profiles(PROFILES, loci)
    assert table == {("1", "12", "3"): "10", ("2", "7", "4"): "11"}                                  # clonal_complex ignored; loci in the scheme's order; the first row of two wins
    assert lt.parse_profiles(PROFILES.encode(), loci) == table
    for bad, word in (("", "empty"), ("id\tadk\n", "ST column"), ("ST\tadk\tfumC\n1\t1\t1\n", "gyrB"), ("ST\tadk\tfumC\tgyrB\n1\t1\n", "columns")):
        with pytest.raises(ValueError, match=word):
            lt.parse_profiles(bad, loci)
    rows = [[m[l][c] for l in range(3)] for c in range(5)]
    assert [lt.assign_st(table, r) for r in rows] == ["10", "11", "-", "-", "novel"]          # a partial call and a missing one: "-"; exact everywhere, no row: novel
    names = ["s0", "s\t1", "s2", "gone", None]
    res = lt.result(loci, lc, sc, rec, lambda c: names[c], excluded=[3], call_matrix=m, profiles=table)
    assert list(res) == ["loci", "samples"] and res["loci"][0] == {"name": "adk", "records": 2, "called": 4, "exact": 3, "multiple": 1}
    assert [s["colour"] for s in res["samples"]] == [0, 1, 2, 4] and [s["ST"] for s in res["samples"]] == ["10", "11", "-", "novel"]
    assert res["samples"][2] == {"sample_name": "s2", "colour": 2, "called": 2, "exact": 1, "ST": "-",
                                 "calls": {"adk": m[0][2], "fumC": {"allele": "7", "fraction": 1.0, "exact": True, "n_hits": 3}}}
    assert json.loads(lt.to_json(res)) == res
    frac = "%.4f" % ((4 * 0xFFFFFFFF // 9) / 0xFFFFFFFF)
    assert lt.to_tsv(res).split("\n") == ["sample\tST\tadk\tfumC\tgyrB", "s0\t10\t1\t12\t3", "s 1\t11\t2\t7\t4", "s2\t-\t2~" + frac + "\t7\t-", "None\tnovel\t1\t12\t4"]
    plain = lt.result(loci, lc, sc, rec, lambda c: names[c], excluded=[3], call_matrix=m)
    assert all("ST" not in s for s in plain["samples"]) and lt.to_tsv(plain).split("\n")[:2] == ["sample\tadk\tfumC\tgyrB", "s0\t1\t12\t3"]
    summary = lt.result(loci, lc, sc, rec, lambda c: names[c], excluded=[3])
    assert all("calls" not in s and "ST" not in s for s in summary["samples"]) and summary["loci"] == res["loci"]
    assert lt.to_tsv(summary, summary_only=True).split("\n") == [
        "locus\trecords\tcalled\texact\tmultiple", "adk\t2\t4\t3\t1", "fumC\t2\t4\t4\t1", "gyrB\t2\t3\t3\t0",
        "sample\tcolour\tcalled\texact", "s0\t0\t3\t3", "s 1\t1\t3\t3", "s2\t2\t2\t1", "None\t4\t3\t3"]


class _FakeIndex(object):
    def __init__(self):
        self.asked = None

    def type_samples(self, scheme, threshold=1.0, profiles=None, summary_only=False, loci_map=None):
        from bigsi_amd import locus_typing as lt
        self.asked = (scheme, threshold, profiles, summary_only, loci_map)
        best, hits, lc, sc, rec = _case()
        table = lt.parse_profiles(profiles, ["adk", "fumC", "gyrB"]) if profiles is not None else None
        return lt.result(["adk", "fumC", "gyrB"], lc, sc, rec, lambda c: "s%d" % c, [3], None if summary_only else lt.calls(best, ALLELES, hits), table)


def test_cli_parsing_text_and_refusals(tmp_path, capsys):
    from bigsi_amd import locus_typing as lt
    from bigsi_amd.__main__ import build_parser, main, typing_text
    p = build_parser()[0]
    a = p.parse_args(["typing", "scheme.fa", "-c", "c.yaml"])
    assert (a.cmd, a.scheme, a.loci_map, a.profiles, a.threshold, a.format, a.summary_only, a.config) == ("typing", "scheme.fa", None, None, 1.0, "tsv", False, "c.yaml")
    a = p.parse_args(["typing", "scheme.fa", "--loci-map", "m.tsv", "--profiles", "p.tsv", "-t", "0.8", "--format", "json", "--summary-only"])
    assert (a.loci_map, a.profiles, a.threshold, a.format, a.summary_only) == ("m.tsv", "p.tsv", 0.8, "json", True)
    for argv in (["typing"], ["typing", "s.fa", "--format", "csv"], ["typing", "s.fa", "-t", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    p.format_help()
    ix = _FakeIndex()
    text = typing_text(ix, "x", 0.5)
    assert ix.asked == ("x", 0.5, None, False, None) and text.split("\n")[:2] == ["sample\tadk\tfumC\tgyrB", "s0\t1\t12\t3"]
    text = typing_text(ix, "x", profiles=PROFILES, loci_map={"a": "b"})
    assert ix.asked == ("x", 1.0, PROFILES, False, {"a": "b"}) and text.split("\n")[1] == "s0\t10\t1\t12\t3"
    assert json.loads(typing_text(ix, "x", fmt="json"))["samples"][0]["calls"]["adk"]["allele"] == "1"
    text = typing_text(ix, "x", summary_only=True)
    assert ix.asked[3] is True and text == lt.to_tsv(ix.type_samples("x", summary_only=True), True) and "calls" not in typing_text(ix, "x", 1.0, "json", True)
    # refused before any device call: --sharded, a threshold above 1, files that cannot be read, an empty scheme, a record without a locus, profiles without a locus's column
    good, empty, odd, prof = tmp_path / "s.fa", tmp_path / "empty.fa", tmp_path / "odd.fa", tmp_path / "p.tsv"
    good.write_text(">adk_1\nAAAA\n>fumC_2\nCCCC\n")
    empty.write_text("")
    odd.write_text(">adk\nAAAA\n")
    prof.write_text("ST\tadk\n1\t1\n")
    for argv, words in ((["typing", str(good), "--sharded"], ("--sharded", "typing")), (["typing", str(good), "-t", "1.5"], ("threshold",)),
                        (["typing", str(tmp_path / "missing.fa")], ("scheme",)), (["typing", str(empty)], ("no record",)), (["typing", str(odd)], ("no locus",)),
                        (["typing", str(good), "--loci-map", str(tmp_path / "missing.tsv")], ("scheme",)), (["typing", str(good), "--profiles", str(prof)], ("fumC",))):
        with pytest.raises(SystemExit):
            main(argv)
        err = capsys.readouterr().err
        assert all(w in err for w in words), (argv, err)


def test_typing_arrays_checks_its_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    for records, lo, nl, kw, err in (("ACGT", [0], 1, {}, TypeError), (["ACGT"], [0], 1, {"threshold": 1.5}, ValueError), (["ACGT"], [0, 1], 1, {}, ValueError),
                                     (["ACGT"], [0], 0, {}, ValueError), (["ACGT"], [1], 1, {}, ValueError), (["ACGT"], [0], 1, {"cell_bytes": 0}, ValueError),
                                     (["ACGT"], [0], 1, {"allele_of": [0xFFFFFFFF]}, ValueError), (["ACGT"], [0], 1, {"allele_of": [0, 1]}, ValueError),
                                     ([b"ACGT"], [0], 1, {}, ValueError), (["ACGé"], [0], 1, {}, ValueError)):
        with pytest.raises(err):
            b.typing_arrays(records, lo, nl, **kw)
    for scheme in ("", ">adk\nACGT\n"):
        with pytest.raises(ValueError):
            b.type_samples(scheme)
    with pytest.raises(ValueError, match="fumC"):
        b.type_samples(">adk_1\nACGT\n>fumC_1\nACGT\n", profiles="ST\tadk\n1\t1\n")


def test_abi_lists_the_new_entry_points():
    from bigsi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_typing.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.TYPING_SIGNATURES) == ["bigsi_hip_typing_add_batch", "bigsi_hip_typing_add_stream", "bigsi_hip_typing_create",
                                                          "bigsi_hip_typing_destroy", "bigsi_hip_typing_fetch", "bigsi_hip_typing_reset"]
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip.h")).read(), flags=re.S)
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.TYPING_SIGNATURES[name][1] and _lib.TYPING_SIGNATURES[name][0] is C.c_int
        assert all(name not in t for t in (_lib.SIGNATURES, _lib.TALLY_SIGNATURES, _lib.CLASSIFY_SIGNATURES, _lib.ASSOCIATE_SIGNATURES, _lib.WINDOW_SIGNATURES,
                                           _lib.KMERCOUNT_SIGNATURES, _lib.COMPACT_SIGNATURES, _lib.FOLD_SIGNATURES, _lib.PREVALENCE_SIGNATURES, _lib.COLLAPSE_SIGNATURES,
                                           _lib.CONSENSUS_SIGNATURES, _lib.PAIRWISE_SIGNATURES, _lib.GENOTYPE_SIGNATURES))
        assert name not in core
    assert "bigsi_hip_typing.h" in open(os.path.join(ROOT, "include", "bigsi_hip.h")).read()          # the LAYERS comment names the header
    n_args = {name: len(sig[1]) for name, sig in _lib.TYPING_SIGNATURES.items()}
    assert n_args == {"bigsi_hip_typing_create": 4, "bigsi_hip_typing_destroy": 1, "bigsi_hip_typing_reset": 1, "bigsi_hip_typing_add_batch": 5,
                      "bigsi_hip_typing_add_stream": 8, "bigsi_hip_typing_fetch": 8}
    twin = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_cpu_typing.h")).read(), flags=re.S)
    assert re.findall(r"\b(bigsi_cpu_\w+)\s*\(", twin) == ["bigsi_cpu_typing"] and len(TWIN_ARGS) == 17
    assert len(re.search(r"bigsi_cpu_typing\s*\((.*?)\)", twin, flags=re.S).group(1).split(",")) == 17
    assert hasattr(C.CDLL(LIB), "bigsi_cpu_typing")
    import bigsi_amd
    assert os.path.exists(os.path.join(os.path.dirname(bigsi_amd.__file__), "locus_typing.py")) and not os.path.exists(os.path.join(os.path.dirname(bigsi_amd.__file__), "typing.py"))


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planner_key_and_twin(tmp_path):
    """tests/c_host/typing_sanitize_main.cpp -- a program with its own main that drives plan_typing, typing_key, the label validation
    and the twin's bigsi_cpu_typing over the refused arguments and the width edges -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a process of its own."""
    exe = str(tmp_path / "typing_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "typing_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "typing planner, key and twin: ok", (r.stdout[-1000:], r.stderr[-3000:])
