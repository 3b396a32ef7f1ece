"""Consensus collapse on the device: bigsi_hip_consensus_columns_into (k_consensus_columns<8 / 16 / 32>) against numpy on the very
bits written with set_rows -- counts[g] = bits[:, group_of == g].sum(axis=1), out[:, g] = counts[g] >= need[g], bit-exact, read back at
the packed width and at the full stride over a preset pattern so that the padding is seen to be zero and no junk from behind the
source's last column to have been counted --, against the OR collapse where every group needs 1, and BIGSI.consensus and the
`consensus` command on top of it.  A wavefront owns whole rows and an LDS image of packed counters for one destination window; the
shapes cross the row grid, the three field widths, fields at their maximum beside each other, the threshold itself and the window
(read from the host planner as committed, not assumed)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import ROOT
from raw_index import Raw, ptr, ragged_bits, rand_seq
from test_collapse_columns_host import DROPPED, collapse_maps, junk_rows
from test_compact_columns_host import WIDTHS
from test_consensus_columns_host import NEVER, consensus_rows, constants, need_vectors, plan, plan_lib, runs_of_255  # noqa: F401 (plan_lib: a fixture)
from test_gpu_collapse_columns import K, M, N_SAMPLES, config, searches, state_of, world_groups

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = -1, -6


def source(bits):
    """An index holding `bits`, written at the full stride with random junk behind the last column."""
    m, n = bits.shape
    a = Raw(m=m, n=n)
    a.write(junk_rows(bits, int(a.info().row_stride_bytes)))
    return a


def consensus(dst, src_handle, group_of, groups, need):
    return dst.L.bigsi_hip_consensus_columns_into(dst.ix, src_handle, ptr(group_of), groups, ptr(need))


def check_consensus(src, bits, group_of, groups, need, ctx, against_collapse=False):
    """The consensus of the resident `src` (which holds `bits`) gives numpy's rows, zero from column G to the end of the stride."""
    m = bits.shape[0]
    dst = Raw(m=m, n=0, cap=1)
    try:
        assert consensus(dst, src.ix, group_of, groups, need) == 0, (ctx, dst.L.bigsi_hip_last_error())
        assert dst.info().num_cols == groups and dst.info().col_capacity >= groups, ctx
        full = dst.rows()
        assert np.array_equal(full, consensus_rows(bits, group_of, groups, need, full.shape[1])), ctx
        rb = (groups + 7) // 8
        assert np.array_equal(dst.rows(row_bytes=rb), full[:, :rb]), ctx
        if against_collapse:          # every group needs 1: the OR collapse of the same source and map, bit for bit
            orr = Raw(m=m, n=0, cap=1)
            try:
                assert orr.L.bigsi_hip_collapse_columns_into(orr.ix, src.ix, ptr(group_of), groups) == 0, orr.L.bigsi_hip_last_error()
                assert orr.info().num_cols == groups and np.array_equal(orr.rows(), full), ctx
            finally:
                orr.close()
    finally:
        dst.close()


def check_all(bits, cases, ctx):
    """cases: [(label, group_of, G)], each with its three need vectors, over one resident source that must stay as it was."""
    src = source(bits)
    try:
        before = src.rows()
        for label, group_of, groups in cases:
            for which, need in need_vectors(group_of, groups):
                check_consensus(src, bits, group_of, groups, need, (ctx, label, which), against_collapse=which == "one")
        assert np.array_equal(src.rows(), before) and src.info().num_cols == bits.shape[1], ctx
    finally:
        src.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_a_widths_and_maps(n):
    check_all(ragged_bits(257, n), collapse_maps(n), n)


@pytest.mark.parametrize("m", [1, 2, 4099])
def test_b_row_counts_around_the_grid(m):
    """One row and two (fewer wavefronts per workgroup than four), and 4099 rows: 1024 workgroups whose wavefronts take a second row."""
    n = 1000
    bits = ragged_bits(m, n) if m > 2 else (np.random.default_rng(m).random((m, n)) < 0.5).astype(np.uint8)
    check_all(bits, [c for c in collapse_maps(n) if c[0] in ("permutation", "many", "emptygroups")], m)


@pytest.mark.parametrize("density", [0.0, 1.0, 0.02])
def test_c_row_densities(density):
    """All-zero rows, all-one rows and sparse rows over three groups -- 1667 members each: 16-bit fields, and every lane meets the
    others in three counters -- and over groups of exactly 255 consecutive columns: 8-bit fields that the all-one rows fill to their
    maximum beside each other, where one add more would carry into the neighbour."""
    m, n = 37, 5000
    bits = (np.random.default_rng(3).random((m, n)) < density).astype(np.uint8)
    check_all(bits, [("three", (np.arange(n) % 3).astype(np.uint32), 3), ("runs255",) + runs_of_255(n)], density)


def test_d_threshold_edges():
    """One group of 300 members (16-bit fields) beside a group of 7; rows with exactly need - 1, need and need + 1 members set."""
    n, size = 320, 300
    rng = np.random.default_rng(4)
    group_of = np.full(n, DROPPED, np.uint32)
    members = np.sort(rng.permutation(n)[:size + 7])
    group_of[members[:size]] = 1
    group_of[members[size:]] = 0
    needs = (1, 2, 150, 299, 300, 301)
    counts = sorted({k for need in needs for k in (need - 1, need, need + 1) if 0 <= k <= size})
    bits = (rng.random((len(counts), n)) < 0.5).astype(np.uint8)
    for r, k in enumerate(counts):          # row r: exactly k members of the large group
        bits[r, members[:size]] = 0
        bits[r, rng.permutation(members[:size])[:k]] = 1
    src = source(bits)
    try:
        for need in needs:
            vec = np.array([3, need], np.uint32)
            dst = Raw(m=len(counts), n=0, cap=1)
            try:
                assert consensus(dst, src.ix, group_of, 2, vec) == 0, dst.L.bigsi_hip_last_error()
                got = np.unpackbits(dst.rows(), axis=1)
                assert got[:, 1].tolist() == [int(k >= need) for k in counts], need
                assert np.array_equal(dst.rows(), consensus_rows(bits, group_of, 2, vec, dst.stride)), need
            finally:
                dst.close()
    finally:
        src.close()


@pytest.mark.parametrize("largest", [255, 256, 65_535, 65_536])
def test_e_field_widths(plan_lib, largest):
    """The largest group at both sides of 8 | 16 and of 16 | 32 bits per field, the others small; rows of density 1.0, 0.5 and 0.03."""
    rng = np.random.default_rng(largest)
    small = 4001
    n, groups = largest + small, 613
    group_of = np.concatenate([np.full(largest, 300, np.uint32), rng.integers(0, 300, small).astype(np.uint32)])[rng.permutation(n)]
    p = plan(plan_lib, n, group_of, groups, tables=False)
    assert (p["field_bits"], p["largest"]) == ({255: 8, 256: 16, 65_535: 16, 65_536: 32}[largest], largest)
    bits = (rng.random((3, n)) < np.array([[1.0], [0.5], [0.03]])).astype(np.uint8)
    check_all(bits, [("largest", group_of, groups)], largest)


def test_f_several_windows(plan_lib):
    """G spans more than three windows of the planner as committed, the last one ragged.  At 8-bit fields: 3 x 16 384 + 77 groups, a
    strided permutation of the first G columns with the others merged into groups of their own choosing.  At 32-bit fields: one
    group of 65 536 members and 3 x 4096 + 77 small ones."""
    k = constants(plan_lib)
    rng = np.random.default_rng(8)
    w8 = k["window_words"] * 64 // 8
    groups, m = 3 * w8 + 77, 5
    n = groups + 6710
    perm = ((np.arange(groups, dtype=np.uint64) * np.uint64(104729)) % np.uint64(groups)).astype(np.uint32)
    assert np.unique(perm).size == groups                                # (104729 is prime and does not divide G)
    group_of = np.concatenate([perm, rng.integers(0, groups, n - groups).astype(np.uint32)])
    p = plan(plan_lib, n, group_of, groups, m=m, tables=False)
    assert p["field_bits"] == 8 and p["windows"] == 4 and p["dst_words"] % p["window_words"] not in (0, p["window_words"] - 1)
    check_all((rng.random((m, n)) < 0.3).astype(np.uint8), [("8-bit", group_of, groups)], "windows")
    w32 = k["window_words"] * 64 // 32
    big, smalls, m = 65_536, 3 * w32 + 77, 3
    groups = smalls + 1
    n = big + smalls + 900
    group_of = np.concatenate([np.full(big, 5000, np.uint32), np.setdiff1d(np.arange(groups, dtype=np.uint32), [5000]),
                               rng.integers(0, groups, 900).astype(np.uint32)]).astype(np.uint32)[rng.permutation(n)]
    p = plan(plan_lib, n, group_of, groups, m=m, tables=False)
    assert p["field_bits"] == 32 and p["windows"] == 4 and p["dst_words"] % p["window_words"] not in (0, p["window_words"] - 1)
    check_all((rng.random((m, n)) < np.array([[1.0], [0.5], [0.1]])).astype(np.uint8), [("32-bit", group_of, groups)], "windows")


def test_g_views_as_source_and_refusals():
    bits = ragged_bits(300, 200)
    label, group_of, groups = collapse_maps(200)[4]
    need = need_vectors(group_of, groups)[2][1]
    a, dst, other_m, other_h, full = source(bits), Raw(m=300, n=0, cap=1), Raw(m=301, n=0, cap=1), Raw(m=300, n=0, cap=1), Raw.from_bits(bits)
    L = a.L
    a.lib.check(L.bigsi_hip_set_num_hashes(other_h.ix, 2))
    view, dst_view = C.c_void_p(), C.c_void_p()
    a.lib.check(L.bigsi_hip_open_view(a.ix, C.byref(view)))
    a.lib.check(L.bigsi_hip_open_view(dst.ix, C.byref(dst_view)))
    bad = group_of.copy()
    bad[141] = groups + 5
    zero = need.copy()
    zero[5] = 0
    call = L.bigsi_hip_consensus_columns_into
    try:
        before = a.rows()
        for fn, want, words in ((lambda: consensus(dst, None, group_of, groups, need), ERR_INVALID, ()),
                                (lambda: call(None, a.ix, ptr(group_of), groups, ptr(need)), ERR_INVALID, ()),
                                (lambda: call(other_m.ix, a.ix, None, groups, ptr(need)), ERR_INVALID, ()),
                                (lambda: call(other_h.ix, a.ix, ptr(group_of), groups, None), ERR_INVALID, ("NULL",)),          # NULL min_members
                                (lambda: consensus(other_m, a.ix, group_of, groups, need), ERR_INVALID, ("301", "300")),
                                (lambda: consensus(other_h, a.ix, group_of, groups, need), ERR_INVALID, ("2", "3")),
                                (lambda: consensus(other_h, a.ix, group_of, 0, need), ERR_INVALID, ("0",)),
                                (lambda: consensus(other_h, a.ix, group_of, 0xFFFFFFFF, need), ERR_INVALID, ("4294967295",)),
                                (lambda: consensus(a, a.ix, group_of, groups, need), ERR_INVALID, ()),                          # dst == src
                                (lambda: consensus(dst, dst_view, group_of, groups, need), ERR_INVALID, ("view",)),             # src a view of dst
                                (lambda: call(view, full.ix, ptr(group_of), groups, ptr(need)), ERR_STATE, ("read-only",)),     # dst a view
                                (lambda: consensus(dst, a.ix, group_of, groups, need), ERR_STATE, ("view",)),                   # dst an owner with a view open
                                (lambda: consensus(full, a.ix, group_of, groups, need), ERR_STATE, ("200",))):                  # dst holds columns
            rc = fn()
            msg = L.bigsi_hip_last_error().decode()
            assert rc == want and msg and all(w in msg for w in words), (rc, want, msg)
        a.lib.check(L.bigsi_hip_close(dst_view))
        dst_view = None
        rc = consensus(dst, a.ix, bad, groups, need)                                                                     # names the column and the value
        msg = L.bigsi_hip_last_error().decode()
        assert rc == ERR_INVALID and "141" in msg and str(groups + 5) in msg
        rc = consensus(dst, a.ix, group_of, groups, zero)                                                                # names the group
        msg = L.bigsi_hip_last_error().decode()
        assert rc == ERR_INVALID and "min_members[5]" in msg
        for r in (dst, other_m, other_h):          # a refused call left the destination empty
            assert r.info().num_cols == 0 and not r.rows().any()
        assert np.array_equal(full.rows(row_bytes=25), np.packbits(bits, axis=1)) and full.info().num_cols == 200
        assert np.array_equal(a.rows(), before) and a.info().num_cols == 200 == a.info(view).num_cols
        # a view AS THE SOURCE works
        assert consensus(dst, view, group_of, groups, need) == 0, L.bigsi_hip_last_error()
        got = dst.rows()
        assert np.array_equal(got, consensus_rows(bits, group_of, groups, need, got.shape[1])) and dst.info().num_cols == groups
    finally:
        for v in (view, dst_view):
            if v is not None:
                a.lib.check(L.bigsi_hip_close(v))
        for r in (a, dst, other_m, other_h, full):
            r.close()


def test_h_an_ipc_handle_is_a_source_and_no_destination():
    """An index attached over hipIpc in a child process (a fresh one): the consensus is taken from there into an index of the child's
    own; as a destination it is refused."""
    bits = ragged_bits(60, 100)
    a = Raw.from_bits(bits)
    try:
        handle = np.zeros(64, np.uint8)
        a.lib.check(a.L.bigsi_hip_export_ipc(a.ix, ptr(handle)))
        code = ("import ctypes as C, sys, numpy as np\n"
                "sys.path.insert(0, %r)\n"
                "from bigsi_amd import _lib\n"
                "L = _lib.lib(); h = np.frombuffer(bytes.fromhex(%r), np.uint8).copy(); ix, dst, own = C.c_void_p(), C.c_void_p(), C.c_void_p()\n"
                "_lib.check(L.bigsi_hip_open_ipc(h.ctypes.data_as(C.c_void_p), 60, 100, 1024, 3, 0, C.byref(ix)))\n"
                "_lib.check(L.bigsi_hip_open(60, 0, 1, 3, 0, C.byref(dst)))\n"
                "_lib.check(L.bigsi_hip_open(60, 5, 5, 3, 0, C.byref(own)))\n"
                "g = (np.arange(100) %% 7).astype(np.uint32); g[::9] = 0xFFFFFFFF\n"
                "need = np.array([1, 2, 5, 9, 12, 13, 14], np.uint32)\n"
                "five, one = np.zeros(5, np.uint32), np.ones(1, np.uint32)\n"
                "rc = [L.bigsi_hip_consensus_columns_into(dst, ix, g.ctypes.data_as(C.c_void_p), 7, need.ctypes.data_as(C.c_void_p))]\n"
                "out = np.zeros((60, 128), np.uint8); ids = np.arange(60, dtype=np.uint64)\n"
                "_lib.check(L.bigsi_hip_get_rows(dst, ids.ctypes.data_as(C.c_void_p), 60, out.ctypes.data_as(C.c_void_p), 128))\n"
                "rc.append(L.bigsi_hip_consensus_columns_into(ix, own, five.ctypes.data_as(C.c_void_p), 1, one.ctypes.data_as(C.c_void_p)))\n"
                "print(rc[0], rc[1], out.tobytes().hex())\n"
                "for x in (ix, dst, own): _lib.check(L.bigsi_hip_close(x))\n") % (ROOT, handle.tobytes().hex())
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        rc0, rc1, rows = r.stdout.split()
        assert (int(rc0), int(rc1)) == (0, ERR_STATE)
        g = (np.arange(100) % 7).astype(np.uint32)
        g[::9] = DROPPED
        need = np.array([1, 2, 5, 9, 12, 13, 14], np.uint32)
        want = consensus_rows(bits, g, 7, need, 128)
        assert np.array_equal(np.frombuffer(bytes.fromhex(rows), np.uint8).reshape(60, 128), want) and 0 < int(np.unpackbits(want).sum()) < 60 * 7
        assert np.array_equal(a.rows(row_bytes=13), np.packbits(bits, axis=1)) and a.info().num_cols == 100
    finally:
        a.close()


# --------------------------------------------------------------------------------------------- BIGSI level
def threshold_filter(filters, members, need):
    """The Bloom filter that keeps a bit where at least `need` of the members' filters have it (need = len(members): their AND)."""
    from bigsi_amd.bitrow import BitRow
    count = np.zeros((M + 7) // 8 * 8, np.int64)
    for n in members:
        count += np.unpackbits(np.frombuffer(filters[n].tobytes(), np.uint8))
    return BitRow.frombytes(np.packbits(count >= need).tobytes(), M)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """70 samples (the colours cross a 64-column word), each a mutated copy of one base sequence that keeps at least base[:80], so
    that every sample -- and so the core of every group -- holds the k-mers of base[:80] (both queries find every core: the 60
    k-mers of base[:70] exactly, 70 of the 150 of base[:160] at threshold 0.4); their Bloom filters from BIGSI.bloom are what a fresh
    build is made of."""
    from bigsi_amd import BIGSI
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(79)
    base = rand_seq(rng, 240)
    seqs = {}
    for c in range(N_SAMPLES):
        cut = int(rng.integers(80, 200))
        seqs["s%d" % c] = base[:cut] + rand_seq(rng, 240 - cut)
    d = tmp_path_factory.mktemp("consensus")
    cfg = config(d, "main")
    b = BIGSI.build_from_sequences(cfg, {n: [s] for n, s in seqs.items()})
    filters = {n: BIGSI.bloom(cfg, list(seq_to_kmers(s, K))) for n, s in seqs.items()}
    made = [b]
    yield {"b": b, "cfg": cfg, "dir": d, "seqs": seqs, "filters": filters, "base": base, "queries": [base[:70], base[:160]], "made": made}
    for x in made:
        x.delete()


def same_index(a, b):
    (kv1, rows1), (kv2, rows2) = state_of(a), state_of(b)
    return kv1 == kv2 and np.array_equal(rows1, rows2)


def test_i_consensus_equals_a_fresh_build_of_the_thresholded_filters(world):
    from bigsi_amd import BIGSI
    from bigsi_amd.consensus import need_of
    b, d, q = world["b"], world["dir"], world["queries"]
    groups = world_groups()
    names = list(groups)
    before = state_of(b)
    for percent in (100, 60):
        new = b.consensus(config(d, "core%d" % percent), groups, percent=percent)
        need = need_of([len(groups[g]) for g in names], percent)
        assert need.tolist() == ([10, 20, 1, 4, 12] if percent == 100 else [6, 12, 1, 3, 8])
        fresh = BIGSI.build(config(d, "core%dfresh" % percent), [threshold_filter(world["filters"], groups[g], int(k)) for g, k in zip(names, need)], names)
        world["made"] += [new, fresh]
        assert new.num_samples == len(names) and [new.colour_to_sample(c) for c in range(len(names))] == names
        assert same_index(new, fresh), percent
        got = searches(new, q)
        assert got == searches(fresh, q) and len(got[0]) == len(names) == len(got[1]), percent
        if percent == 100:          # what every sample holds, every group's core holds: no false negatives for core k-mers
            assert sorted(r["sample_name"] for r in new.search(world["base"][:60])) == sorted(names)
            assert len(b.search(world["base"][:60])) == N_SAMPLES
    # percent=1: the OR of groups of up to 100 members, which is collapse()
    low, orr = b.consensus(config(d, "core1"), groups, percent=1), b.collapse(config(d, "core1or"), groups)
    world["made"] += [low, orr]
    assert same_index(low, orr) and searches(low, q) == searches(orr, q)
    # the source is as it was
    after = state_of(b)
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and b.num_samples == N_SAMPLES


def test_j_keep_others_and_deleted_samples(world):
    from bigsi_amd import BIGSI
    b, d = world["b"], world["dir"]
    groups = world_groups()
    with pytest.raises(ValueError):
        b.consensus(dict(config(d, "never"), m=M + 1), groups)
    for bad, err in (({"A": ["nobody"]}, KeyError), ({"A": ["s1"], "B": ["s1"]}, ValueError), ({}, ValueError)):
        with pytest.raises(err):
            b.consensus(config(d, "never"), bad)
    with pytest.raises(ValueError):
        b.consensus(config(d, "never"), groups, percent=0)
    b.delete_sample("s3")          # a member of "odd"...
    b.delete_sample("s41")         # ... and an unlisted sample
    with pytest.raises(KeyError):
        b.consensus(config(d, "never"), groups)                           # a deleted name
    groups["odd"].remove("s3")
    new = b.consensus(config(d, "others"), groups, percent=80, keep_others=True)
    world["made"].append(new)
    listed = {s for ms in groups.values() for s in ms}
    rest = ["s%d" % c for c in range(N_SAMPLES) if "s%d" % c not in listed and c not in (3, 41)]
    names = list(groups) + rest
    assert [new.colour_to_sample(c) for c in range(new.num_samples)] == names and new.num_samples == len(names) == 5 + 22
    members = [groups[g] for g in groups] + [[s] for s in rest]          # a sample kept on its own needs 1: it is copied
    fresh = BIGSI.build(config(d, "othersfresh"), [threshold_filter(world["filters"], ms, max(1, -(-80 * len(ms) // 100))) for ms in members], names)
    world["made"].append(fresh)
    assert same_index(new, fresh)
    assert searches(new, world["queries"]) == searches(fresh, world["queries"])


def test_k_groups_are_refused(tmp_path):
    from bigsi_amd import BIGSI
    from bigsi_amd._lib import BigsiHipError
    rng = np.random.default_rng(10)
    cfg = config(tmp_path, "grp")
    cfg["storage-config"].update(devices=[0, 0], max_cols=8)
    del cfg["storage-config"]["filename"]
    b = BIGSI.build_from_sequences(cfg, {"g%d" % c: [rand_seq(rng, 60)] for c in range(6)})
    try:
        for call in (lambda: b.consensus(config(tmp_path, "never"), {"A": ["g1", "g2"]}),
                     lambda: b.storage.consensus_columns_into(b.storage, np.zeros(6, np.uint32), 1, np.ones(1, np.uint32))):
            with pytest.raises(BigsiHipError) as e:
                call()
            assert e.value.code == ERR_STATE
        assert b.num_samples == 6
    finally:
        b.delete()


def test_l_cli_consensus_then_search(tmp_path, capsys):
    """`python -m bigsi_amd consensus` in a process of its own on an index's snapshot, then a `search` under the new config (through
    the same main(), on the snapshot the child left) that sees the cores: what both members of a group hold is found, what one of
    them holds alone is not."""
    from bigsi_amd import BIGSI
    from bigsi_amd.__main__ import main
    from bigsi_amd.storage.hip_hbm import HipHbmStorage
    rng = np.random.default_rng(12)
    cfg, to = config(tmp_path, "cli"), config(tmp_path, "clito")
    shared = {"A": rand_seq(rng, 60), "B": rand_seq(rng, 60)}
    group = {"c0": "A", "c5": "A", "c2": "B", "c6": "B"}
    seqs = {"c%d" % c: [shared.get(group.get("c%d" % c), "") + rand_seq(rng, 90)] for c in range(7)}
    b = BIGSI.build_from_sequences(cfg, seqs)
    b.delete_sample("c4")
    b.storage.sync()
    HipHbmStorage.drop(cfg["storage-config"]["name"])                     # (the snapshot is what the child process sees)
    cf, tf, gf = tmp_path / "config.yaml", tmp_path / "to.yaml", tmp_path / "groups.tsv"
    cf.write_text(yaml.safe_dump(cfg))
    tf.write_text(yaml.safe_dump(to))
    gf.write_text("c6\tB\nc0\tA\nc2\tB\n\nc5\tA\n")
    r = subprocess.run([sys.executable, "-m", "bigsi_amd", "consensus", str(tf), "--groups", str(gf), "--percent", "100", "--config", str(cf)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    try:
        assert json.loads(r.stdout) == {"result": "consensus of 4 of 6 samples from %s at 100 %% into 2 groups in %s." % (cf, tf), "groups": 2, "samples_in": 6,
                                        "samples_dropped": 2, "num_samples": 2, "members": {"B": ["c2", "c6"], "A": ["c0", "c5"]}, "percent": 100,
                                        "min_members": {"B": 2, "A": 2}}
        for name in ("A", "B"):
            capsys.readouterr()
            assert main(["search", shared[name][:50], "--config", str(tf)]) == 0
            assert [x["sample_name"] for x in json.loads(capsys.readouterr().out)["results"]] == [name]
        capsys.readouterr()
        assert main(["search", seqs["c5"][0][70:130], "--config", str(tf)]) == 0          # held by one member only: not in the core
        assert json.loads(capsys.readouterr().out)["results"] == []
        new = BIGSI(to)
        assert [new.colour_to_sample(c) for c in range(new.num_samples)] == ["B", "A"]
    finally:
        for c in (to, cfg):
            if os.path.exists(c["storage-config"]["filename"]):
                BIGSI(c).delete()
