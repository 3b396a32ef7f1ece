"""Row folding without a GPU: the identity it rests on, the host-only helpers of bigsi_amd/fold.py, the CPU twin of
bigsi_hip_fold_rows / bigsi_hip_fold_rows_into / bigsi_hip_trim_rows against numpy on the rows written and against a twin index BUILT
under the smaller filter size, the ABI of the new headers, and plan_fold_rows (csrc/bigsi_launch.hpp, compiled by g++)."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raw_index import junk_rows, ptr, rand_seq
from test_compact_columns_host import Info
from test_cpu_twin import Index

LIB = os.path.join(ROOT, "bigsi_amd", "libbigsi_cpu.so")
ERR_INVALID, ERR_STATE = -1, -6
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def divisors(m):
    return [d for d in range(1, m + 1) if m % d == 0]


# --------------------------------------------------------------------------------------------- the identity
@pytest.mark.parametrize("m", [7 * 3, 1000, 1024, 2 * 3 * 5 * 7 * 11])
def test_floor_mod_identity_for_every_divisor(m):
    """row = floor_mod(signed 32-bit hash, m) (Python's % IS floor_mod); for every divisor d the row under m, reduced mod m' = m / d,
    is the row under m' -- so ORing the d rows that share a residue is the build under m'."""
    rng = np.random.default_rng(m)
    hashes = [0, -1, 1, INT32_MIN, INT32_MIN + 1, INT32_MAX, INT32_MAX - 1, m, -m, m - 1, 1 - m] + [int(x) for x in rng.integers(INT32_MIN, INT32_MAX, 500, endpoint=True)]
    for d in divisors(m):
        new_m = m // d
        for x in hashes:
            assert 0 <= x % m < m
            assert (x % m) % new_m == x % new_m, (m, d, x)


# --------------------------------------------------------------------------------------------- bigsi_amd/fold.py
def test_fold_plan():
    from bigsi_amd.fold import fold_plan
    assert fold_plan(1000, 8) == 125 and fold_plan(1000, 1) == 1000 and fold_plan(1000, 1000) == 1 and fold_plan(25_000_015, 5) == 5_000_003
    for bad in (0, 3, 7, 1001, -2):
        with pytest.raises(ValueError) as e:
            fold_plan(1000, bad)
        assert str(bad) in str(e.value) and "1000" in str(e.value)          # both numbers in the message
    for bad in (2.0, "2", None, True, False, np.float64(2)):
        with pytest.raises(TypeError):
            fold_plan(1000, bad)
    with pytest.raises(TypeError):
        fold_plan(True, 1)


def test_divisors_near():
    from bigsi_amd.fold import divisors, divisors_near
    assert divisors(1000) == [1, 2, 4, 5, 8, 10, 20, 25, 40, 50, 100, 125, 200, 250, 500, 1000]
    m = 25_000_015          # = 5 x 83 x 107 x 563
    assert divisors(m) == sorted({a * b * c * d for a in (1, 5) for b in (1, 83) for c in (1, 107) for d in (1, 563)})
    near = divisors_near(m, m // 2)
    assert near[0] == (5, 5_000_003) and all(m % f == 0 and f > 1 and f * r == m for f, r in near) and len(near) == 5
    assert near == sorted(near)
    assert divisors_near(1000, 100) == [(8, 125), (10, 100), (20, 50), (25, 40), (40, 25)]
    assert divisors_near(1000, 100, count=1) == [(10, 100)]
    assert divisors_near(1009, 500) == [(1009, 1)]          # a prime: only m' = 1
    assert divisors_near(1, 1) == []
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            divisors_near(1000, bad)


def test_fold_estimate_formula():
    from bigsi_amd.fold import fold_estimate, fold_estimate_rows
    assert fold_estimate([0, 1000], 1000, 3, 2) == [(0.0, 0.0), (1.0, 1.0)]
    (f, p), = fold_estimate([100], 1000, 3, 2)
    assert f == pytest.approx(1 - 0.9 ** 2, rel=1e-15) and p == pytest.approx(f ** 3, rel=1e-15)
    assert fold_estimate([250], 1000, 2, 1) == [(0.25, 0.0625)]
    for args in (([1], 1000, 3, 3), ([1001], 1000, 3, 2), ([1], 1000, 0, 2), ([-1], 1000, 3, 2)):
        with pytest.raises(ValueError):
            fold_estimate(*args)
    rows = fold_estimate_rows([{"sample_name": "a", "colour": 0, "bits_set": 100, "fill": 0.1, "kmer_fpr": 0.001, "est_kmers": 35.1}], 1000, 3, 2)
    assert list(rows[0]) == ["sample_name", "colour", "bits_set", "fill", "est_fill", "est_kmer_fpr"] and rows[0]["est_fill"] == f


@pytest.mark.parametrize("m,d,fill", [(60000, 2, 0.3), (60000, 8, 0.05), (65536, 16, 0.01), (50050, 5, 0.5), (30030, 3, 0.9)])
def test_fold_estimate_against_folded_random_columns(m, d, fill):
    """The model against what folding does to independent random bits.  A folded bit is set with probability p = 1 - (1 - X/m)^d
    given the column's own popcount X only approximately (the X set bits are a sample without replacement), so the bound is taken
    from the binomial model the estimate states: the folded popcount of m' independent bits has standard deviation
    sqrt(m' p (1 - p)); 6 sigma of it, computed here from m' and the predicted fill, bounds |folded popcount - m' p|.  (Sampling
    without replacement only narrows the spread.)  Seeds are fixed: the test was run on the model alone and passes."""
    from bigsi_amd.fold import fold_estimate
    rng = np.random.default_rng(m * 31 + d)
    new_m = m // d
    cols = rng.random((m, 40)) < fill
    est = fold_estimate(cols.sum(axis=0).tolist(), m, 3, d)
    folded = np.bitwise_or.reduce(cols.reshape(d, new_m, 40), axis=0).sum(axis=0)
    for c in range(40):
        p = est[c][0]
        sigma = math.sqrt(new_m * p * (1 - p))
        assert abs(int(folded[c]) - new_m * p) <= 6 * sigma, (c, int(folded[c]), new_m * p, sigma)
        assert est[c][1] == pytest.approx(p ** 3, rel=1e-15)


# --------------------------------------------------------------------------------------------- the CPU twin
@pytest.fixture(scope="module")
def cpu():
    assert os.path.exists(LIB), "libbigsi_cpu.so has not been built (run __graft_entry__.build())"
    L = C.CDLL(LIB)
    L.bigsi_cpu_last_error.restype = C.c_char_p
    return L


def twin_open(L, m, n, cap=None, h=3):
    ix = C.c_void_p()
    assert L.bigsi_cpu_open(C.c_uint64(m), C.c_uint64(n), C.c_uint64(cap or max(n, 1)), C.c_uint32(h), 0, C.byref(ix)) == 0
    return ix


def twin_write(L, ix, packed):
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    ids = np.arange(packed.shape[0], dtype=np.uint64)
    assert L.bigsi_cpu_set_rows(ix, ptr(ids), C.c_uint64(ids.size), ptr(packed), C.c_uint64(packed.shape[1])) == 0, L.bigsi_cpu_last_error()


def twin_rows(L, ix, m, row_bytes):
    out = np.full((m, row_bytes), 0xAB, np.uint8)
    ids = np.arange(m, dtype=np.uint64)
    assert L.bigsi_cpu_get_rows(ix, ptr(ids), C.c_uint64(m), ptr(out), C.c_uint64(row_bytes)) == 0, L.bigsi_cpu_last_error()
    return out


def twin_info(L, ix):
    inf = Info()
    assert L.bigsi_cpu_get_info(ix, C.byref(inf)) == 0
    return inf


def expected_fold(packed, d, n, out_bytes):
    """numpy on the very bytes written: the OR over the d row groups, cut to n columns, zero up to out_bytes."""
    m = packed.shape[0]
    folded = np.bitwise_or.reduce(packed.reshape(d, m // d, packed.shape[1]), axis=0)
    bits = np.unpackbits(folded, axis=1)[:, :n]
    want = np.zeros((m // d, out_bytes), np.uint8)
    if n:
        want[:, :(n + 7) // 8] = np.packbits(bits, axis=1)
    return want


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("new_m", [1, 7, 64, 65])
def test_twin_against_numpy(cpu, new_m, cols):
    rng = np.random.default_rng(new_m * 1000 + cols)
    for d in (1, 2, 3, 5, 8, 9, 16, 17):
        m = new_m * d
        ix = twin_open(cpu, m, cols)
        stride = int(twin_info(cpu, ix).row_stride_bytes)
        packed = junk_rows(rng, m, cols, stride)
        twin_write(cpu, ix, packed)
        src = twin_open(cpu, m, cols)
        twin_write(cpu, src, packed)
        got_m = C.c_uint64(0)
        assert cpu.bigsi_cpu_fold_rows(ix, C.c_uint64(d), C.byref(got_m)) == 0, cpu.bigsi_cpu_last_error()
        inf = twin_info(cpu, ix)
        assert got_m.value == new_m == inf.num_rows and inf.num_cols == cols and inf.index_bytes == new_m * stride
        want = expected_fold(packed, d, cols, stride) if d > 1 else packed          # factor 1 touches nothing, junk included
        assert np.array_equal(twin_rows(cpu, ix, new_m, stride), want), (new_m, d, cols)
        ids = np.array([new_m], np.uint64)
        assert cpu.bigsi_cpu_get_rows(ix, ptr(ids), C.c_uint64(1), ptr(np.zeros(stride, np.uint8)), C.c_uint64(stride)) != 0          # rows >= m' are gone
        # out of place, into a destination of another stride; factor 1 is a copy (through the fold: junk dropped)
        dst = twin_open(cpu, new_m, 0, cap=1 if cols < 1000 else 3000)
        assert cpu.bigsi_cpu_fold_rows_into(dst, src) == 0, cpu.bigsi_cpu_last_error()
        dinf = twin_info(cpu, dst)
        assert dinf.num_cols == cols and dinf.num_rows == new_m
        assert np.array_equal(twin_rows(cpu, dst, new_m, int(dinf.row_stride_bytes)), expected_fold(packed, d, cols, int(dinf.row_stride_bytes))), (new_m, d, cols)
        assert np.array_equal(twin_rows(cpu, src, m, stride), packed)          # the source is only read
        for h in (ix, src, dst):
            assert cpu.bigsi_cpu_close(h) == 0


def test_twin_error_paths_and_trim(cpu):
    rng = np.random.default_rng(3)
    packed = junk_rows(rng, 60, 100, 128)
    a, empty7, empty60, full, other_h = twin_open(cpu, 60, 100), twin_open(cpu, 7, 0), twin_open(cpu, 30, 0), twin_open(cpu, 30, 5), twin_open(cpu, 30, 0, h=2)
    twin_write(cpu, a, packed)
    for call, want, words in ((lambda: cpu.bigsi_cpu_fold_rows(None, C.c_uint64(2), None), ERR_INVALID, ()),
                            (lambda: cpu.bigsi_cpu_fold_rows(a, C.c_uint64(0), None), ERR_INVALID, ("0", "60")),
                            (lambda: cpu.bigsi_cpu_fold_rows(a, C.c_uint64(7), None), ERR_INVALID, ("7", "60")),
                            (lambda: cpu.bigsi_cpu_fold_rows(a, C.c_uint64(120), None), ERR_INVALID, ("120", "60")),
                            (lambda: cpu.bigsi_cpu_fold_rows_into(None, a), ERR_INVALID, ()),
                            (lambda: cpu.bigsi_cpu_fold_rows_into(empty60, None), ERR_INVALID, ()),
                            (lambda: cpu.bigsi_cpu_fold_rows_into(a, a), ERR_INVALID, ()),                        # dst == src
                            (lambda: cpu.bigsi_cpu_fold_rows_into(empty7, a), ERR_INVALID, ("7", "60")),          # 60 / 7 is no integer
                            (lambda: cpu.bigsi_cpu_fold_rows_into(a, empty60), ERR_INVALID, ("60", "30")),        # the ratio is below 1
                            (lambda: cpu.bigsi_cpu_fold_rows_into(other_h, a), ERR_INVALID, ("2", "3")),          # num_hashes differ
                            (lambda: cpu.bigsi_cpu_fold_rows_into(full, a), ERR_STATE, ("5",)),                   # non-empty dst
                            (lambda: cpu.bigsi_cpu_trim_rows(None), ERR_INVALID, ())):
        rc = call()
        msg = cpu.bigsi_cpu_last_error().decode()
        assert rc == want and msg and all(w in msg for w in words), (rc, want, msg)
    assert np.array_equal(twin_rows(cpu, a, 60, 128), packed) and twin_info(cpu, a).num_rows == 60          # a refused call changed nothing
    # factor 1: a no-op (new_num_rows may be NULL); trim with nothing to gain: a no-op
    assert cpu.bigsi_cpu_fold_rows(a, C.c_uint64(1), None) == 0 and cpu.bigsi_cpu_trim_rows(a) == 0
    assert np.array_equal(twin_rows(cpu, a, 60, 128), packed)
    # fold, then trim: the same bytes; a second fold of the folded index is one fold by the product
    assert cpu.bigsi_cpu_fold_rows(a, C.c_uint64(2), None) == 0
    want = expected_fold(packed, 2, 100, 128)
    assert np.array_equal(twin_rows(cpu, a, 30, 128), want)
    assert cpu.bigsi_cpu_trim_rows(a) == 0 and cpu.bigsi_cpu_trim_rows(a) == 0
    assert np.array_equal(twin_rows(cpu, a, 30, 128), want) and twin_info(cpu, a).num_rows == 30
    assert cpu.bigsi_cpu_fold_rows(a, C.c_uint64(3), None) == 0
    assert np.array_equal(twin_rows(cpu, a, 10, 128), expected_fold(packed, 6, 100, 128))
    # a trimmed index grows again as any other (reserve_cols sizes the new table by the rows the index has now)
    assert cpu.bigsi_cpu_reserve_cols(a, C.c_uint64(5000)) == 0
    assert np.array_equal(twin_rows(cpu, a, 10, 128), expected_fold(packed, 6, 100, 128))
    for h in (a, empty7, empty60, full, other_h):
        assert cpu.bigsi_cpu_close(h) == 0


K, H = 11, 3


@pytest.mark.parametrize("m", [2 * 3 * 5 * 7, 1024])
def test_twin_folded_index_equals_the_index_built_under_the_smaller_size(cpu, m):
    """A twin index built under m from seeded sequences, folded by each divisor, IS the twin index built under m / d: row bytes,
    searches at thresholds 1.0 and 0.4, lookups -- and the oracle's model of the reference at m / d agrees."""
    from oracle.ref_model import OracleBIGSI, seq_to_kmers
    rng = np.random.default_rng(m)
    base = rand_seq(rng, 120)
    seqs = [base[:int(rng.integers(30, 110))] + rand_seq(rng, 40) for _ in range(9)]
    queries = [base[:40], base[:100], seqs[3][-30:]]
    names = ["s%d" % c for c in range(len(seqs))]

    def build(rows):
        ix = Index(cpu, rows, H, len(seqs))
        for c, s in enumerate(seqs):
            ix.add_sample(c, [s], K)
        return ix

    def answers(ix, rows):
        out = [ix.rows(2).tobytes()]
        for thr in (1.0, 0.4):
            nk, nu, mk, ho, col, cnt = ix.search(queries, K, thr)
            out.append((nk.tolist(), nu.tolist(), mk.tolist(), ho.tolist(), col.tolist(), cnt.tolist()))
        kmers = sorted(set(seq_to_kmers(queries[1], K)))
        look = np.zeros((len(kmers), 2), np.uint8)
        ix.ok(cpu.bigsi_cpu_lookup(ix.ix, "".join(kmers).encode(), C.c_uint32(K), C.c_uint64(len(kmers)), ptr(look)))
        out.append(look.tobytes())
        return out

    for d in divisors(m):
        if d == 1:
            continue
        new_m = m // d
        folded, rebuilt = build(m), build(new_m)
        assert cpu.bigsi_cpu_fold_rows(folded.ix, C.c_uint64(d), None) == 0, cpu.bigsi_cpu_last_error()
        folded.m = new_m
        got, want = answers(folded, new_m), answers(rebuilt, new_m)
        assert got == want, (m, d)
        model = OracleBIGSI.build([OracleBIGSI.bloom(seq_to_kmers(s, K), new_m, H) for s in seqs], names, K, new_m, H)
        assert model.rows.tobytes() == got[0], (m, d)
        for q, thr, rec in ((0, 1.0, got[1]), (1, 0.4, got[2])):
            ho, col, cnt = rec[3], rec[4], rec[5]
            mine = sorted(zip(col[ho[q]:ho[q + 1]], cnt[ho[q]:ho[q + 1]]), key=lambda x: (-x[1], x[0]))
            ref = [(names.index(r["sample_name"]), r["num_kmers_found"]) for r in model.search(queries[q], thr)]
            assert mine == sorted(ref, key=lambda x: (-x[1], x[0])), (m, d, q)
        folded.close()
        rebuilt.close()


# --------------------------------------------------------------------------------------------- ABI
def header_names(name, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % prefix, src)))


def test_abi_of_the_new_headers(tmp_path):
    from bigsi_amd import _lib
    new = ["bigsi_hip_fold_rows", "bigsi_hip_fold_rows_into", "bigsi_hip_trim_rows"]
    assert header_names("bigsi_hip_fold.h", "bigsi_hip_") == sorted(_lib.FOLD_SIGNATURES) == new
    for name in new:
        assert getattr(_lib.lib(), name).argtypes == _lib.FOLD_SIGNATURES[name][1]
        assert name not in _lib.SIGNATURES and name not in _lib.COMPACT_SIGNATURES
    for other in ("bigsi_hip.h", "bigsi_hip_compact.h", "bigsi_hip_group.h", "bigsi_hip_testing.h", "bigsi_hip_text.h"):
        assert not set(new) & set(header_names(other, "bigsi_hip_")), other
    assert sorted(_lib.COMPACT_SIGNATURES) == ["bigsi_hip_compact_columns", "bigsi_hip_extract_columns", "bigsi_hip_shrink_to_fit"]
    # the twin mirrors it: the same parameter lists (handle type aside), the renaming macros, exported symbols
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)      # noqa: E731
    decl = lambda src, prefix: {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\b%s(\w+)\s*\(([^;{]*?)\)\s*;" % prefix, src)}      # noqa: E731
    cpu_h, hip_h = open(os.path.join(ROOT, "include", "bigsi_cpu_fold.h")).read(), open(os.path.join(ROOT, "include", "bigsi_hip_fold.h")).read()
    c, h = decl(strip(cpu_h), "bigsi_cpu_"), decl(strip(hip_h), "bigsi_hip_")
    assert sorted(c) == sorted(h) == ["fold_rows", "fold_rows_into", "trim_rows"]
    L = C.CDLL(LIB)
    for name, params in c.items():
        assert params.replace("bigsi_cpu_index", "bigsi_hip_index") == h[name]
        assert "#define bigsi_hip_%s bigsi_cpu_%s" % (name, name) in cpu_h and hasattr(L, "bigsi_cpu_" + name)
    # both headers are C99
    for hdr in ("bigsi_hip_fold.h", "bigsi_cpu_fold.h"):
        src = tmp_path / ("use_%s.c" % hdr[:-2])
        src.write_text('#include "%s"\nint main(void) { return bigsi_hip_fold_rows(0, 2, 0) == BIGSI_OK; }\n' % hdr)
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


# --------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fold_host") / "libfold_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "c_host", "fold_host.cpp")])
    return C.CDLL(so)


PLAN_KEYS = ("block", "seg_groups", "rows_per_step", "rows_per_block", "row_blocks", "grid", "loads", "max_loads", "waves", "min_rows")


def plan(lib, new_m, d, stride):
    out = np.zeros(10, np.uint64)
    lib.fold_host_plan(C.c_uint64(new_m), C.c_uint64(d), C.c_uint64(stride), ptr(out))
    return dict(zip(PLAN_KEYS, (int(x) for x in out)))


def check_plan(p, new_m, d, stride):
    segs = max(-(-stride // 128), 1)
    assert p["block"] % 64 == 0 and 64 <= p["block"] <= 256 and p["seg_groups"] * (p["block"] // 64) >= segs > (p["seg_groups"] - 1) * (p["block"] // 64)
    # the row blocks [b * rows_per_block, min((b + 1) * rows_per_block, m')) cover [0, m') exactly once, and none is empty
    assert p["rows_per_block"] >= 1 and p["row_blocks"] >= 1
    assert (p["row_blocks"] - 1) * p["rows_per_block"] < new_m <= p["row_blocks"] * p["rows_per_block"]
    assert p["grid"] == p["seg_groups"] * p["row_blocks"] < 1 << 31
    # a block is whole steps; the register budget: rows per step x loads per row <= kFoldMaxLoads, and >= kFoldLoads loads where d < kFoldLoads
    assert p["rows_per_block"] % p["rows_per_step"] == 0
    per_row = min(d, p["loads"])
    assert p["rows_per_step"] * per_row <= p["max_loads"] == 16 and p["loads"] == 8
    assert p["rows_per_step"] * per_row >= p["loads"] and (p["rows_per_step"] - 1) * per_row < p["loads"]
    # about kFoldWaves wavefronts, fewer only for a matrix smaller than the target: blocks of at least min_rows rows
    want_blocks = max(p["waves"] // segs, 1)
    assert p["row_blocks"] <= want_blocks
    if new_m >= want_blocks * (p["min_rows"] + p["rows_per_step"]):
        assert p["row_blocks"] * 2 > want_blocks          # (rounding a block up to whole steps costs at most a few blocks)
    else:
        assert p["rows_per_block"] <= p["min_rows"] + p["rows_per_step"] + new_m // want_blocks


def test_plan_fold_rows_over_seeded_shapes(plan_lib):
    rng = np.random.default_rng(2024)
    shapes = [(1, 2, 16), (1, 1000, 16), (7, 3, 16), (64, 2, 16), (65, 2, 16), (66, 3, 16), (67, 3, 16), (4099, 17, 320), (5_000_000, 2, 1568), (12_500_000, 2, 992),
              (1_250_000, 8, 1568), (1 << 40, 2, 16), (1 << 33, 7, 1 << 26), (3, 1 << 40, 1 << 26)]
    for _ in range(4000):
        new_m = int(rng.integers(1, 1 << int(rng.integers(1, 36))))
        d = int(rng.integers(1, 1 << int(rng.integers(1, 12))))
        stride = 16 * int(rng.integers(1, 1 << int(rng.integers(1, 22))))
        shapes.append((new_m, d, min(stride, 1 << 26)))
    for new_m, d, stride in shapes:
        check_plan(plan(plan_lib, new_m, d, stride), new_m, d, stride)


def test_plan_fold_rows_pinned_shapes(plan_lib):
    """The shapes the GPU tests lean on (a block is 64 rows, 66 for a factor of 3) and the two the measurement runs."""
    for (new_m, d, stride), want in (((1, 2, 16), (64, 1, 4, 64, 1, 1)), ((64, 2, 16), (64, 1, 4, 64, 1, 1)), ((65, 2, 16), (64, 1, 4, 64, 2, 2)),
                                     ((66, 3, 16), (64, 1, 3, 66, 1, 1)), ((67, 3, 16), (64, 1, 3, 66, 2, 2)), ((4099, 17, 320), (192, 1, 1, 64, 65, 65)),
                                     ((4099, 5, 16), (64, 1, 2, 64, 65, 65)), ((5_000_000, 2, 1568), (256, 4, 4, 15876, 315, 1260)),
                                     ((12_500_000, 2, 992), (256, 2, 4, 24416, 512, 1024))):
        p = plan(plan_lib, new_m, d, stride)
        assert tuple(p[k] for k in PLAN_KEYS[:6]) == want, ((new_m, d, stride), p)


# --------------------------------------------------------------------------------------------- decided before any device call
def test_fold_checks_its_arguments_first():
    """(there is no storage here: whatever raises did so before touching one)"""
    from bigsi_amd.graph.bigsi import BIGSI
    b = BIGSI.__new__(BIGSI)
    b.bloomfilter_size, b.num_hashes, b.config = 1000, 3, {"k": 11}
    for bad in (1, "yes", None):
        with pytest.raises(TypeError):
            b.fold(2, trim=bad)
    for bad, err in ((0, ValueError), (3, ValueError), (2.0, TypeError), (True, TypeError)):
        with pytest.raises(err):
            b.fold(bad)
        with pytest.raises(err):
            b.fold_into({"m": 500, "h": 3, "k": 11}, bad)
    for cfg in ({"m": 501, "h": 3, "k": 11}, {"m": 500, "h": 2, "k": 11}, {"m": 500, "h": 3, "k": 13}):
        with pytest.raises(ValueError):
            b.fold_into(cfg, 2)


def test_cli_parsing_and_in_place_check():
    from bigsi_amd.__main__ import build_parser, fold_check_in_place, main
    p = build_parser()[0]
    a = p.parse_args(["fold", "new.yaml", "--factor", "4", "-c", "c.yaml"])
    assert (a.cmd, a.to_config, a.factor, a.in_place, a.dry_run, a.no_trim, a.format) == ("fold", "new.yaml", 4, False, False, False, "json")
    a = p.parse_args(["fold", "--factor", "2", "--dry-run", "--format", "csv"])
    assert a.to_config is None and a.dry_run and a.format == "csv"
    assert p.parse_args(["fold", "n.yaml", "--factor", "2", "--in-place", "--no-trim"]).in_place
    with pytest.raises(SystemExit):
        p.parse_args(["fold", "n.yaml"])          # --factor is required
    cfg = {"storage-engine": "hip-hbm", "m": 1000, "h": 3, "k": 11, "storage-config": {"name": "x", "filename": "x.hbm"}}
    assert fold_check_in_place(cfg, dict(cfg, m=250), 4) == 250
    for bad in (dict(cfg, m=500), dict(cfg, m=250, h=2), dict(cfg, m=250, k=9), dict(cfg, m=250, **{"storage-config": {"name": "y", "filename": "x.hbm"}}),
                dict(cfg, m=250, **{"storage-config": {"name": "x", "filename": "y.hbm"}})):
        with pytest.raises(ValueError):
            fold_check_in_place(cfg, bad, 4)
    with pytest.raises(ValueError):
        fold_check_in_place(cfg, dict(cfg, m=250), 3)


def test_cli_refuses_sharded_and_a_missing_target(capsys, tmp_path):
    import yaml
    from bigsi_amd.__main__ import main
    cf = tmp_path / "c.yaml"
    cf.write_text(yaml.safe_dump({"storage-engine": "hip-hbm", "m": 1000, "h": 3, "k": 11, "storage-config": {"name": "never-opened"}}))
    for argv, word in ((["fold", "to.yaml", "--factor", "2", "--sharded", "-c", str(cf)], "--sharded"), (["fold", "--factor", "2", "-c", str(cf)], "TO_CONFIG")):
        with pytest.raises(SystemExit):
            main(argv)
        assert word in capsys.readouterr().err


class _FakeIndex(object):
    bloomfilter_size, num_hashes = 1000, 3

    def sample_stats(self):
        return [{"sample_name": "a", "colour": 0, "bits_set": 100, "fill": 0.1, "kmer_fpr": 0.001, "est_kmers": 35.1},
                {"sample_name": "b", "colour": 2, "bits_set": 0, "fill": 0.0, "kmer_fpr": 0.0, "est_kmers": 0.0}]


def test_cli_dry_run_text():
    from bigsi_amd.__main__ import fold_dry_run_text
    out = json.loads(fold_dry_run_text(_FakeIndex(), 8))
    assert list(out) == ["m", "factor", "valid", "new_m", "factors_near", "note", "estimate"]
    assert (out["m"], out["factor"], out["valid"], out["new_m"]) == (1000, 8, True, 125) and [8, 125] in out["factors_near"] and "estimate" in out["note"]
    assert [r["sample_name"] for r in out["estimate"]] == ["a", "b"] and out["estimate"][0]["est_fill"] == pytest.approx(1 - 0.9 ** 8)
    assert out["estimate"][0]["est_kmer_fpr"] == pytest.approx((1 - 0.9 ** 8) ** 3) and out["estimate"][1]["est_fill"] == 0.0
    out = json.loads(fold_dry_run_text(_FakeIndex(), 7))          # not a divisor: the factors that exist, no table
    assert out["valid"] is False and out["new_m"] is None and out["estimate"] == [] and all(1000 % f == 0 for f, _ in out["factors_near"])
    lines = fold_dry_run_text(_FakeIndex(), 2, "csv").split("\n")
    assert lines[0] == "sample_name,colour,bits_set,fill,est_fill,est_kmer_fpr" and len(lines) == 3 and lines[1].startswith("a,0,100,0.1,")
