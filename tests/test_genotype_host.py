"""Panel genotyping without a GPU: the conditions the planted cases must hold so that no GPU comparison passes vacuously, the host
planner plan_genotype and the allele_of validation (csrc/bigsi_launch.hpp, compiled by g++) against a plain Python restatement
(tests/genotype_ref.py), the CPU twin bigsi_cpu_genotype against the numpy reference on the planted indexes the GPU tests use, the
host layer (bigsi_amd/genotype.py: parse_panel on the golden panel, slices, calls, result, TSV / JSON), what BIGSI.genotype_arrays
and the command line decide before any device call, the ABI lists, and a stand-alone sanitized program over the planner and the
twin."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import genotype_ref as R
import tally_ref as T
from conftest import ROOT
from raw_index import ptr

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g12_variant.json")
ERR_INVALID, ERR_NOMEM, ERR_CAPACITY, ERR_STATE = -1, -3, -5, -6
PLAN_FIELDS = ("block", "tile", "word_blocks", "tiles", "grid", "variants_grid", "samples_grid", "plane_bytes", "too_large", "bad_variants", "too_many_bytes")


# --------------------------------------------------------------------------------------------- outputs with guards
class Out(object):
    """The five outputs of a fetch, preset to 0xAB, with a guard entry behind each"""

    def __init__(self, n_variants, n_cols):
        self.nv, self.n_cols, self.rb = n_variants, n_cols, (n_cols + 7) // 8
        self.ref, self.alt = np.zeros((n_variants + 1, self.rb), np.uint8), np.zeros((n_variants + 1, self.rb), np.uint8)
        self.variants, self.samples, self.probes = np.zeros((n_variants + 1, 4), np.uint32), np.zeros((n_cols + 1, 2), np.uint32), np.zeros((n_variants + 1, 2), np.uint32)
        for a in self.arrays():
            a.view(np.uint8)[:] = 0xAB

    def arrays(self):
        return (self.ref, self.alt, self.variants, self.samples, self.probes)

    def guards_hold(self):
        return all(a[-1].tobytes() == b"\xab" * a[-1].nbytes for a in self.arrays())

    def untouched(self):
        return all(a.tobytes() == b"\xab" * a.nbytes for a in self.arrays())

    def got(self, planes=True):
        assert self.guards_hold()
        return dict(ref=self.ref[:-1] if planes else None, alt=self.alt[:-1] if planes else None, variants=self.variants[:-1], samples=self.samples[:-1],
                    probes=self.probes[:-1])


def same(got, want, what):
    """the outputs of a fetch against the reference, bit for bit; the calls follow from the planes"""
    for key in ("variants", "samples", "probes", "ref", "alt"):
        if got[key] is None:
            continue
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
        bad = np.argwhere(got[key] != want[key])
        assert bad.size == 0, (what, key, bad[:4].tolist(), [got[key][tuple(i)] for i in bad[:4]], [want[key][tuple(i)] for i in bad[:4]])
    if got["ref"] is not None:
        from bigsi_amd import genotype
        assert np.array_equal(genotype.calls(got["ref"], got["alt"], want["calls"].shape[1]), want["calls"]), (what, "calls")


# --------------------------------------------------------------------------------------------- the reference's own conditions
@pytest.mark.parametrize("n_cols", R.CONDITION_WIDTHS)
def test_cases_cannot_pass_vacuously(n_cols):
    """on the very planted indexes, layouts and thresholds the GPU cases run"""
    p = R.width_case(n_cols)
    thr, i, e = p.edge_threshold()
    assert 0 < thr < 1 and T.min_kmers(int(p.us[i]), thr) == int(p.counts[i, e]) < p.us[i] and R.thresholds(p) == (1.0, thr, 0.0)
    R.check_conditions(p)
    al, w, p1, p2 = R.two_tile_word(p, 1.0)
    assert p1 // R.TILE == 0 and p2 // R.TILE == 1
    assert (-(-n_cols // 64)) % 2 == (0 if n_cols == 200 else 1)          # 775 columns: an odd number of result words, a pad word behind them


def test_panel_and_layouts():
    al, nv = R.alleles(R.N_QUERIES)
    assert nv == R.N_VARIANTS == 28 and al.max() < 2 * nv and not (al >> 1 == R.EMPTY).any()
    assert al[2] == 2 * R.SHORT_ALT + 1 and (al == 2 * R.SHORT_ALT + 1).sum() == 1 and (al == 2 * R.NO_ALT + 1).sum() == 0 and (al == 2 * R.ALT_ONLY).sum() == 0
    assert al[16] == al[64] == 32 and al[1] == 2                                     # variant 16's ref probes lie 48 apart; the zero-hit query is variant 1's ref
    assert al[24] == 1 and al[25] == 2 * 23 + 1 and al[27] == 3                      # even c' -> variant c', odd c' -> variant c' - 2 (mod 24)
    for name in R.LAYOUTS:
        order, a, n = R.layout(name, R.N_QUERIES)
        assert sorted(order.tolist()) == list(range(R.N_QUERIES)) and n == nv
        keep = a != R.NONE
        assert np.array_equal(a[keep], al[order][keep]) and ((~keep).sum() > 0) == (name == "shuffled")
    order, a, _ = R.layout("grouped", R.N_QUERIES)
    assert (np.diff(a.astype(np.int64)) >= 0).all() and not (np.diff(R.layout("interleaved", R.N_QUERIES)[1].astype(np.int64)) >= 0).all()
    al, nv = R.alleles(9, 65)
    assert nv == 65 and al.tolist() == [0, 2, 4, 6, 8, 10, 12, 14, 16]
    al, nv = R.alleles(9, 2)
    assert al.tolist() == [0, 2, 1, 3, 0, 2, 1, 3, 0]


def test_genotype_of_is_the_definition():
    """a second statement of the definition: genotypes() of bigsi_amd/variant_search.py over the names of the hit columns"""
    from bigsi_amd.variant_search import genotypes
    p = R.width_case(200)
    columns, drop = R.column_mask(p)
    for thr in R.thresholds(p) + (-0.5,):
        hit = R.hits_of(p, thr)
        for name in R.LAYOUTS:
            for masked in (False, True):
                order, al, nv = R.layout(name, len(p.seqs))
                g = R.genotype_of(p.us, hit, order, al, nv, columns if masked else None)
                live = [c for c in range(200) if not (masked and c == drop)]
                for v in range(nv):
                    ref_names = [c for q in (order[i] for i in range(len(order)) if al[i] == 2 * v) for c in live if hit[q, c]]
                    alt_names = [c for q in (order[i] for i in range(len(order)) if al[i] == 2 * v + 1) for c in live if hit[q, c]]
                    want = {r["sample_name"]: r["genotype"] for r in genotypes(ref_names, alt_names)}
                    got = {c: ("0/0", "0/1", "1/1")[g["calls"][v, c]] for c in range(200) if g["calls"][v, c] != 3}
                    assert got == want, (thr, name, masked, v)
                    assert g["variants"][v].tolist() == [sum(x == s for x in want.values()) for s in ("0/0", "0/1", "1/1")] + [len(live) - len(want)]
                carried = [(g["calls"][:, c] == 1).sum() + (g["calls"][:, c] == 2).sum() for c in range(200)]
                assert g["samples"][:, 0].tolist() == carried and g["samples"][:, 1].tolist() == [(g["calls"][:, c] != 3).sum() for c in range(200)]
                assert np.array_equal(np.unpackbits(g["ref"], axis=1)[:, :200] | np.unpackbits(g["alt"], axis=1)[:, :200], (g["calls"] != 3).astype(np.uint8))
    a, b = R.genotype_of(p.us, R.hits_of(p, -0.5), order, al, nv), R.genotype_of(p.us, R.hits_of(p, 0.0), order, al, nv)
    assert all(np.array_equal(a[k], b[k]) for k in a)


# --------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("genotype_host") / "libgenotype_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "genotype_host.cpp")])
    lib = C.CDLL(so)
    lib.genotype_host_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.genotype_host_bad_allele.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    lib.genotype_host_bad_allele.restype = C.c_uint64
    return lib


def compiled_plan(lib, n_seqs, wv, n_variants):
    out = np.zeros(len(PLAN_FIELDS), np.uint64)
    lib.genotype_host_plan(n_seqs, wv, n_variants, ptr(out))
    return dict(zip(PLAN_FIELDS, (int(x) for x in out)))


def test_constants_are_the_restated_ones(plan_lib):
    c = np.zeros(7, np.uint64)
    plan_lib.genotype_host_constants(ptr(c))
    assert [int(x) for x in c] == [R.BLOCK, R.NONE, R.MAX_VARIANTS, R.PLANE_BYTES, R.TILE, R.LOADS, T.CHUNK_SEQS]
    assert R.TILE <= R.BLOCK and R.TILE % R.LOADS == 0
    header = open(os.path.join(ROOT, "include", "bigsi_hip_genotype.h")).read()
    assert "#define BIGSI_GENOTYPE_NONE 0xFFFFFFFFu" in header and "#define BIGSI_GENOTYPE_MAX_VARIANTS (1u << 20)" in header
    assert "#define BIGSI_GENOTYPE_PLANE_BYTES (4ull << 30)" in header and "DESIGN limit, not a\n * measured one" in header
    from bigsi_amd import genotype
    assert (genotype.NONE, genotype.MAX_VARIANTS, genotype.GENOTYPES) == (R.NONE, R.MAX_VARIANTS, ("0/0", "0/1", "1/1", "./."))


def test_plan_genotype_against_restatement(plan_lib):
    for n_seqs in (0, 1, 63, 64, 65, 128, 129, 4096, 64 * 0x7FFFFFFF, 64 * 0x7FFFFFFF + 1, 1 << 40):
        for wv in (1, 2, 4, 13, 255, 256, 257, 1563, 15625, 4 * 0x7FFFFFFF, 4 * 0x7FFFFFFF + 1, 1 << 34, 1 << 62):
            for n_variants in (0, 1, 2, 3, 4, 5, 63, 64, 65, 1000, 17179, 17180, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 40):
                p = compiled_plan(plan_lib, n_seqs, wv, n_variants)
                assert p == R.plan_genotype(n_seqs, wv, n_variants), (n_seqs, wv, n_variants)
                assert p["grid"] == min(-(-wv // 256) * -(-n_seqs // 64), (1 << 64) - 1) and p["bad_variants"] == (not 1 <= n_variants <= 1 << 20)
                if not p["bad_variants"]:
                    assert p["too_many_bytes"] == (16 * n_variants * wv > 4 << 30) and p["variants_grid"] == -(-n_variants // 4)
                    assert p["plane_bytes"] == (0 if p["too_many_bytes"] else 16 * n_variants * wv)
    # grids above 2^31 - 1 are refused; the last one that is not
    assert compiled_plan(plan_lib, 64 * 0x7FFFFFFF, 1, 1)["too_large"] == 0 and compiled_plan(plan_lib, 64 * 0x7FFFFFFF + 1, 1, 1)["too_large"] == 0x80000000
    assert compiled_plan(plan_lib, 1, 4 * 0x7FFFFFFF, 1)["too_large"] == 0 and compiled_plan(plan_lib, 1, 4 * 0x7FFFFFFF + 1, 1)["too_large"] == 0x80000000
    assert compiled_plan(plan_lib, 65 * 64, 1 << 33, 1)["too_large"] == 65 << 25 and compiled_plan(plan_lib, 1 << 40, 1 << 62, 1)["too_large"] == (1 << 64) - 1
    # the 4 GiB design limit: both planes of all variants, in whole words -- a million samples (15625 words) take 17179 variants, not 17180
    assert compiled_plan(plan_lib, 1, 15625, 17179)["too_many_bytes"] == 0 and compiled_plan(plan_lib, 1, 15625, 17180)["too_many_bytes"] == 1
    assert compiled_plan(plan_lib, 1, 256, 1 << 20)["plane_bytes"] == 4 << 30 and compiled_plan(plan_lib, 1, 257, 1 << 20)["too_many_bytes"] == 1
    assert compiled_plan(plan_lib, 1, 1 << 62, 1 << 20) == R.plan_genotype(1, 1 << 62, 1 << 20)          # (the product does not fit 64 bits)


def test_allele_validation(plan_lib):
    a = np.array([0, 1, 5, R.NONE, 4], np.uint32)
    bad = plan_lib.genotype_host_bad_allele
    assert bad(ptr(a), 5, 3) == 5 and bad(ptr(a), 5, 2) == 2 and bad(ptr(a), 2, 1) == 2 and bad(ptr(a), 5, 1) == 2 and bad(ptr(a), 0, 1) == 0
    a[2] = 0xFFFFFFFE
    assert bad(ptr(a), 5, 1 << 20) == 2 and bad(ptr(a), 5, 1 << 31) == 5


# --------------------------------------------------------------------------------------------- the CPU twin
TWIN_ARGS = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
             C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]


@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    L.bigsi_cpu_genotype.argtypes = TWIN_ARGS
    L.bigsi_cpu_genotype.restype = C.c_int32
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


def twin_genotype(L, ix, n_cols, seqs, thr, allele_of, n_variants, columns=None, planes=True, plane_cap=None, sample_cap=None):
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(seqs)
    out = Out(max(n_variants, 1), n_cols)
    allele_of = np.ascontiguousarray(allele_of, np.uint32)
    rc = L.bigsi_cpu_genotype(ix, blob, ptr(off), len(seqs), T.K, thr, ptr(allele_of), n_variants, ptr(columns), ptr(out.ref) if planes else None,
                              ptr(out.alt) if planes else None, out.nv * out.rb if plane_cap is None else plane_cap, ptr(out.variants), ptr(out.samples),
                              n_cols if sample_cap is None else sample_cap, ptr(out.probes))
    assert out.guards_hold()
    return rc, out


@pytest.mark.parametrize("n_cols", R.WIDTHS)
def test_twin_against_numpy(cpu, n_cols):
    p = R.width_case(n_cols)
    ix = twin_index(cpu, p)
    columns = R.column_mask(p)[0]
    for name in R.LAYOUTS:
        order, al, nv = R.layout(name, len(p.seqs))
        seqs = [p.seqs[q] for q in order]
        for thr in R.thresholds(p):
            for masked in (False, True):
                rc, out = twin_genotype(cpu, ix, n_cols, seqs, thr, al, nv, columns if masked else None)
                assert rc == 0, cpu.bigsi_cpu_last_error()
                same(out.got(), R.planted_genotype(p, thr, name, masked), (n_cols, name, thr, masked))
    rc, out = twin_genotype(cpu, ix, n_cols, seqs, -1.0, al, nv, planes=False)
    assert rc == 0 and out.ref.tobytes() == b"\xab" * out.ref.nbytes and out.alt.tobytes() == b"\xab" * out.alt.nbytes
    same(out.got(planes=False), R.planted_genotype(p, 0.0, name), (n_cols, "a threshold below 0, no planes"))
    assert cpu.bigsi_cpu_close(ix) == 0


def test_twin_refusals(cpu):
    p = R.width_case(65)
    order, al, nv = R.layout("grouped", len(p.seqs))
    seqs = [p.seqs[q] for q in order]
    ix = twin_index(cpu, p)
    bad = al.copy()
    bad[7] = 2 * nv
    for kw, rc_want, word in ((dict(thr=1.5), ERR_INVALID, b"threshold"), (dict(thr=float("nan")), ERR_INVALID, b"threshold"), (dict(n_variants=0), ERR_INVALID, b"BIGSI_GENOTYPE_MAX_VARIANTS"),
                              (dict(n_variants=(1 << 20) + 1), ERR_INVALID, b"BIGSI_GENOTYPE_MAX_VARIANTS"), (dict(allele_of=bad), ERR_INVALID, b"allele_of[7]"),
                              (dict(n_variants=nv - 1), ERR_INVALID, b"allele_of["), (dict(plane_cap=nv * 9 - 1), ERR_CAPACITY, b"plane"),
                              (dict(sample_cap=64), ERR_CAPACITY, b"sample_counts")):
        args = dict(thr=1.0, allele_of=al, n_variants=nv)
        args.update(kw)
        rc, out = twin_genotype(cpu, ix, 65, seqs, args["thr"], args["allele_of"], args["n_variants"], plane_cap=args.get("plane_cap"), sample_cap=args.get("sample_cap"))
        assert rc == rc_want and out.untouched() and word in cpu.bigsi_cpu_last_error(), (kw, cpu.bigsi_cpu_last_error())
    from bigsi_amd._lib import pack_seqs
    blob, off = pack_seqs(seqs)
    out = Out(nv, 65)
    call = cpu.bigsi_cpu_genotype
    tail = (ptr(out.ref), ptr(out.alt), nv * 9, ptr(out.variants), ptr(out.samples), 65, ptr(out.probes))
    head = (blob, ptr(off), len(seqs), T.K, 1.0, ptr(al), nv, None)
    for args in ((None,) + head + tail, (ix, blob, None) + head[2:] + tail, (ix,) + head[:5] + (None, nv, None) + tail,
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
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_parse_panel_on_the_golden_cases():
    from bigsi_amd import genotype
    from bigsi_amd.variant_search import split_probes
    g = golden()
    cases = g["cases"]
    assert len(cases) == 16 and sum(len(c["alts"]) == 3 for c in cases) == 4
    text = "".join(c["probes_fasta"] for c in cases)
    for panel in (text, text.encode()):
        names, probes, allele_of = genotype.parse_panel(panel)
        assert names == [c["query"] for c in cases] and allele_of.dtype == np.uint32 and len(probes) == allele_of.size == sum(len(c["refs"]) + len(c["alts"]) for c in cases)
        assert (np.diff(allele_of.astype(np.int64)) >= 0).all()                      # grouped by allele
        for v, c in enumerate(cases):
            assert [probes[i] for i in np.flatnonzero(allele_of == 2 * v)] == c["refs"] == split_probes(c["probes_fasta"])[0]
            assert [probes[i] for i in np.flatnonzero(allele_of == 2 * v + 1)] == c["alts"] == split_probes(c["probes_fasta"])[1]
    # a variant's ref records may come in several adjacent records, its alts in between; names end at "?" or whitespace
    names, probes, allele_of = genotype.parse_panel(">ref-A1C?x=1\nAAAA\n>alt-A1C-0\nCCCC\n>ref-A1C extra\nGGGG\n>alt-1\nTTTT\n>ref-B2\nAC\nGT\n")
    assert names == ["A1C", "B2"] and probes == ["AAAA", "GGGG", "CCCC", "TTTT", "ACGT"] and allele_of.tolist() == [0, 0, 1, 1, 2]
    assert genotype.parse_panel("")[:2] == ([], []) and genotype.parse_panel("")[2].size == 0
    with pytest.raises(ValueError, match="starts with"):
        genotype.parse_panel(">alt-A1C-0\nCCCC\n>ref-A1C\nAAAA\n")
    with pytest.raises(ValueError, match="twice"):
        genotype.parse_panel(">ref-A\nAAAA\n>ref-B\nCCCC\n>ref-A\nGGGG\n")


def test_panel_file(tmp_path):
    from bigsi_amd import genotype
    f = tmp_path / "panel.fa"
    f.write_text(golden()["cases"][3]["probes_fasta"])
    names, probes, allele_of = genotype.parse_panel(str(f))
    assert names == ["T60X"] and allele_of.tolist() == [0, 1, 1, 1]


def test_slices():
    from bigsi_amd import genotype
    al = np.array([0, 1, 1, 2, R.NONE, 5, 8, 9, 9], np.uint32)
    one = genotype.slices(al, 5, 9, 1 << 30)
    assert len(one) == 1 and one[0][:2] == (0, 5) and one[0][2].tolist() == [0, 1, 2, 3, 5, 6, 7, 8] and one[0][3].tolist() == [0, 1, 1, 2, 5, 8, 9, 9]
    # 9 row bytes are two words: 32 bytes of planes per variant; 64 bytes hold two variants
    got = genotype.slices(al, 5, 9, 64)
    assert [(v0, v1, idx.tolist(), rel.tolist()) for v0, v1, idx, rel in got] == [(0, 2, [0, 1, 2, 3], [0, 1, 1, 2]), (2, 4, [5], [1]), (4, 5, [6, 7, 8], [0, 1, 1])]
    assert [(v0, v1) for v0, v1, _, _ in genotype.slices(al, 5, 9, 1)] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]          # at least one variant each


def _case():
    """three variants over five columns, column 3 deleted: planes, counts as the device would leave them"""
    r = np.array([[1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, 0, 1, 0, 1]], np.uint8)
    a = np.array([[0, 1, 1, 0, 0], [0, 0, 0, 0, 1], [0, 0, 0, 0, 0]], np.uint8)
    vc = np.array([[1, 1, 1, 1], [0, 0, 1, 3], [3, 0, 0, 1]], np.uint32)
    sc = np.array([[0, 2], [1, 1], [1, 2], [0, 0], [1, 2]], np.uint32)
    ap = np.array([[2, 1], [1, 1], [1, 0]], np.uint32)
    return np.packbits(r, axis=1), np.packbits(a, axis=1), vc, sc, ap


def test_calls_result_and_text():
    from bigsi_amd import genotype
    ref, alt, vc, sc, ap = _case()
    m = genotype.calls(ref, alt, 5)
    assert m.dtype == np.uint8 and m.tolist() == [[0, 1, 2, 3, 3], [3, 3, 3, 3, 2], [0, 3, 0, 3, 0]]
    assert genotype.calls(ref | 0x07, alt, 5).tolist() == m.tolist()                  # bits behind the last column are ignored
    assert genotype.calls(ref | 0x10, alt, 5, excluded=[3, 99]).tolist() == m.tolist()          # an excluded column is missing whatever it holds
    names = ["s0", "s\t1", "s2", "gone", None]
    res = genotype.result(["A1C", "B2", "C3"], vc, sc, ap, lambda c: names[c], excluded=[3], call_matrix=m)
    assert list(res) == ["variants", "samples"]
    assert res["variants"][0] == {"name": "A1C", "ref_probes": 2, "alt_probes": 1, "counts": {"0/0": 1, "0/1": 1, "1/1": 1, "./.": 1},
                                  "calls": {"s0": "0/0", "s\t1": "0/1", "s2": "1/1"}}
    assert res["variants"][1]["calls"] == {} and "uncallable" not in res["variants"][1]          # (column 4 has no name: reported by its colour alone)
    assert res["variants"][2] == {"name": "C3", "ref_probes": 1, "alt_probes": 0, "counts": {"0/0": 3, "0/1": 0, "1/1": 0, "./.": 1},
                                  "calls": {"s0": "0/0", "s2": "0/0"}, "uncallable": True}
    assert res["samples"] == [{"sample_name": "s0", "colour": 0, "carried": 0, "called": 2}, {"sample_name": "s\t1", "colour": 1, "carried": 1, "called": 1},
                              {"sample_name": "s2", "colour": 2, "carried": 1, "called": 2}, {"sample_name": None, "colour": 4, "carried": 1, "called": 2}]
    assert json.loads(genotype.to_json(res)) == res
    assert genotype.to_tsv(res).split("\n") == ["variant\ts0\ts 1\ts2\tNone", "A1C\t0/0\t0/1\t1/1\t./.", "B2\t./.\t./.\t./.\t./.", "C3\t0/0\t./.\t0/0\t./."]
    summary = genotype.result(["A1C", "B2", "C3"], vc, sc, ap, lambda c: names[c], excluded=[3])
    assert all("calls" not in v for v in summary["variants"]) and summary["samples"] == res["samples"] and summary["variants"][2]["uncallable"] is True
    assert genotype.to_tsv(summary, summary_only=True).split("\n") == [
        "variant\tref_probes\talt_probes\t0/0\t0/1\t1/1\t./.", "A1C\t2\t1\t1\t1\t1\t1", "B2\t1\t1\t0\t0\t1\t3", "C3\t1\t0\t3\t0\t0\t1",
        "sample\tcolour\tcarried\tcalled", "s0\t0\t0\t2", "s 1\t1\t1\t1", "s2\t2\t1\t2", "None\t4\t1\t2"]


class _FakeIndex(object):
    def __init__(self):
        self.asked = None

    def genotype_panel(self, panel, threshold=1.0, summary_only=False):
        from bigsi_amd import genotype
        self.asked = (panel, threshold, summary_only)
        ref, alt, vc, sc, ap = _case()
        return genotype.result(["A1C", "B2", "C3"], vc, sc, ap, lambda c: "s%d" % c, [3], None if summary_only else genotype.calls(ref, alt, 5))


def test_cli_parsing_text_and_refusals(tmp_path, capsys):
    from bigsi_amd import genotype
    from bigsi_amd.__main__ import build_parser, genotype_text, main
    p = build_parser()[0]
    a = p.parse_args(["genotype", "panel.fa", "-c", "c.yaml"])
    assert (a.cmd, a.panel, a.threshold, a.format, a.summary_only, a.config) == ("genotype", "panel.fa", 1.0, "tsv", False, "c.yaml")
    a = p.parse_args(["genotype", "panel.fa", "-t", "0.8", "--format", "json", "--summary-only"])
    assert (a.threshold, a.format, a.summary_only) == (0.8, "json", True)
    for argv in (["genotype"], ["genotype", "p.fa", "--format", "csv"], ["genotype", "p.fa", "-t", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    p.format_help()
    ix = _FakeIndex()
    text = genotype_text(ix, ">ref-A1C\nAAAA\n", 0.5)
    assert ix.asked == (">ref-A1C\nAAAA\n", 0.5, False) and text.split("\n")[0] == "variant\ts0\ts1\ts2\ts4" and text.split("\n")[1] == "A1C\t0/0\t0/1\t1/1\t./."
    assert json.loads(genotype_text(ix, "x", fmt="json"))["variants"][0]["calls"] == {"s0": "0/0", "s1": "0/1", "s2": "1/1"}
    text = genotype_text(ix, "x", summary_only=True)
    assert ix.asked == ("x", 1.0, True) and text == genotype.to_tsv(ix.genotype_panel("x", summary_only=True), True) and "calls" not in genotype_text(ix, "x", 1.0, "json", True)
    # refused before any device call: --sharded, a threshold above 1, a panel that cannot be read, is empty, or starts with an alt record
    good, empty, alt_first = tmp_path / "p.fa", tmp_path / "empty.fa", tmp_path / "alt.fa"
    good.write_text(">ref-A1C\nAAAA\n>alt-A1C-0\nCCCC\n")
    empty.write_text("")
    alt_first.write_text(">alt-A1C-0\nCCCC\n")
    for argv, words in ((["genotype", str(good), "--sharded"], ("--sharded", "genotype")), (["genotype", str(good), "-t", "1.5"], ("threshold",)),
                        (["genotype", str(tmp_path / "missing.fa")], ("panel",)), (["genotype", str(empty)], ("no variant",)), (["genotype", str(alt_first)], ("starts with",))):
        with pytest.raises(SystemExit):
            main(argv)
        err = capsys.readouterr().err
        assert all(w in err for w in words), (argv, err)


def test_genotype_arrays_checks_its_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    for probes, al, nv, kw, err in (("ACGT", [0], 1, {}, TypeError), (["ACGT"], [0], 1, {"threshold": 1.5}, ValueError), (["ACGT"], [0, 1], 1, {}, ValueError),
                                    (["ACGT"], [0], 0, {}, ValueError), (["ACGT"], [2], 1, {}, ValueError), (["ACGT"], [0], 1, {"plane_bytes": 0}, ValueError),
                                    ([b"ACGT"], [0], 1, {}, ValueError), (["ACGé"], [0], 1, {}, ValueError)):
        with pytest.raises(err):
            b.genotype_arrays(probes, al, nv, **kw)
    for panel in ("", ">alt-x\nACGT\n"):
        with pytest.raises(ValueError):
            b.genotype_panel(panel)


def test_abi_lists_the_new_entry_points():
    from bigsi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip_genotype.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bigsi_hip_\w+)\s*\(", src)))
    assert declared == sorted(_lib.GENOTYPE_SIGNATURES) == ["bigsi_hip_genotype_add_batch", "bigsi_hip_genotype_add_stream", "bigsi_hip_genotype_create",
                                                            "bigsi_hip_genotype_destroy", "bigsi_hip_genotype_fetch", "bigsi_hip_genotype_reset"]
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_hip.h")).read(), flags=re.S)
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == _lib.GENOTYPE_SIGNATURES[name][1] and _lib.GENOTYPE_SIGNATURES[name][0] is C.c_int
        assert all(name not in t for t in (_lib.SIGNATURES, _lib.TALLY_SIGNATURES, _lib.CLASSIFY_SIGNATURES, _lib.ASSOCIATE_SIGNATURES, _lib.WINDOW_SIGNATURES,
                                           _lib.KMERCOUNT_SIGNATURES, _lib.COMPACT_SIGNATURES, _lib.FOLD_SIGNATURES, _lib.PREVALENCE_SIGNATURES, _lib.COLLAPSE_SIGNATURES,
                                           _lib.CONSENSUS_SIGNATURES, _lib.PAIRWISE_SIGNATURES))
        assert name not in core
    assert "bigsi_hip_genotype.h" in open(os.path.join(ROOT, "include", "bigsi_hip.h")).read()          # the LAYERS comment names the header
    n_args = {name: len(sig[1]) for name, sig in _lib.GENOTYPE_SIGNATURES.items()}
    assert n_args == {"bigsi_hip_genotype_create": 4, "bigsi_hip_genotype_destroy": 1, "bigsi_hip_genotype_reset": 1, "bigsi_hip_genotype_add_batch": 4,
                      "bigsi_hip_genotype_add_stream": 7, "bigsi_hip_genotype_fetch": 8}
    twin = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bigsi_cpu_genotype.h")).read(), flags=re.S)
    assert re.findall(r"\b(bigsi_cpu_\w+)\s*\(", twin) == ["bigsi_cpu_genotype"] and len(TWIN_ARGS) == 16
    assert hasattr(C.CDLL(LIB), "bigsi_cpu_genotype")


# --------------------------------------------------------------------------------------------- sanitizers, on the CPU
def test_sanitized_program_over_planner_and_twin(tmp_path):
    """tests/c_host/genotype_sanitize_main.cpp -- a program with its own main that drives plan_genotype, the allele_of validation and
    the twin's bigsi_cpu_genotype at the width edges -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process
    of its own."""
    exe = str(tmp_path / "genotype_san")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",          # (the runtimes are part of the program: no library order to get wrong)
                           "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c_host", "genotype_sanitize_main.cpp"), os.path.join(ROOT, "bigsi_amd", "cpu", "bigsi_cpu.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "genotype planner and twin: ok", (r.stdout[-1000:], r.stderr[-3000:])
