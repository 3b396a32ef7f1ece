"""Column collapse on the device: bigsi_hip_collapse_columns_into (k_collapse_columns) against numpy on the very bits written with
set_rows -- expected[:, g] = bits[:, group_of == g].any(axis=1), bit-exact, read back at the packed width and at the full stride over a
preset pattern so that the padding is seen to be zero and no junk from behind the source's last column to have come along -- and
BIGSI.collapse and the `collapse` command on top of it.  Every column of the matrices differs from its neighbours, so a column that
lands in the wrong place shows.  A wavefront owns whole rows and an LDS image of one destination window; the shapes cross the row
grid, the image's pairs of words and the window (read from the host planner as committed, not assumed)."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import ROOT
from raw_index import Raw, ptr, ragged_bits, rand_seq
from test_collapse_columns_host import DROPPED, collapse_maps, constants, expected_rows, junk_rows, plan, plan_lib  # noqa: F401 (plan_lib: a fixture)
from test_compact_columns_host import WIDTHS, pack_keep

pytestmark = pytest.mark.gpu
_counter = itertools.count()
ERR_INVALID, ERR_STATE = -1, -6


def source(bits):
    """An index holding `bits`, written at the full stride with random junk behind the last column."""
    m, n = bits.shape
    a = Raw(m=m, n=n)
    a.write(junk_rows(bits, int(a.info().row_stride_bytes)))
    return a


def collapse(dst, src_handle, group_of, groups):
    return dst.L.bigsi_hip_collapse_columns_into(dst.ix, src_handle, ptr(group_of), groups)


def check_collapse(bits, group_of, groups, ctx, against_extract=False):
    """The collapse gives numpy's rows, zero from column G to the end of the stride; the source stays as it was."""
    m, n = bits.shape
    src, dst = source(bits), Raw(m=m, n=0, cap=1)
    try:
        before = src.rows()
        assert collapse(dst, src.ix, group_of, groups) == 0, (ctx, dst.L.bigsi_hip_last_error())
        assert dst.info().num_cols == groups and dst.info().col_capacity >= groups, ctx
        full = dst.rows()
        assert np.array_equal(full, expected_rows(bits, group_of, groups, full.shape[1])), ctx
        rb = (groups + 7) // 8
        assert np.array_equal(dst.rows(row_bytes=rb), full[:, :rb]), ctx
        assert np.array_equal(src.rows(), before) and src.info().num_cols == n, ctx
        if against_extract:          # a monotone injective map = the extraction of the same columns
            ext = Raw(m=m, n=0, cap=1)
            try:
                assert ext.L.bigsi_hip_extract_columns(ext.ix, src.ix, ptr(pack_keep(group_of != DROPPED))) == 0, ext.L.bigsi_hip_last_error()
                assert np.array_equal(ext.rows(row_bytes=rb), full[:, :rb]) and ext.info().num_cols == groups, ctx
            finally:
                ext.close()
    finally:
        src.close()
        dst.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_a_widths_and_maps(n):
    bits = ragged_bits(257, n)
    for label, group_of, groups in collapse_maps(n):
        check_collapse(bits, group_of, groups, (n, label), against_extract=label == "monotone")


@pytest.mark.parametrize("m", [1, 2, 4099])
def test_b_row_counts_around_the_grid(m):
    """One row and two (fewer wavefronts per workgroup than four), and 4099 rows: 1024 workgroups whose wavefronts take a second row."""
    n = 1000
    bits = ragged_bits(m, n) if m > 2 else (np.random.default_rng(m).random((m, n)) < 0.5).astype(np.uint8)
    for label, group_of, groups in collapse_maps(n):
        if label in ("permutation", "many", "emptygroups"):
            check_collapse(bits, group_of, groups, (m, label))


@pytest.mark.parametrize("density", [0.0, 1.0, 0.02])
def test_c_row_densities(density):
    """All-zero rows (nothing to walk), all-one rows -- every lane at its longest bit walk, and with 5000 columns in 3 groups every
    LDS word hit by many lanes at once --, and sparse rows."""
    m, n = 37, 5000
    bits = (np.random.default_rng(3).random((m, n)) < density).astype(np.uint8)
    three = (np.arange(n) % 3).astype(np.uint32)
    check_collapse(bits, three, 3, (density, "three"))
    for label, group_of, groups in collapse_maps(n):
        if label in ("many", "reversal"):
            check_collapse(bits, group_of, groups, (density, label))


def test_d_several_windows(plan_lib):
    """G spans more than two windows of the planner as committed, the last one ragged: at the starting window of 2048 words,
    400 003 columns into 393 293 groups.  Once many-to-one (a strided permutation of the first G columns, the others merged into
    groups of their own choosing), once injective (the others dropped): that one equals extract_columns + numpy reordering."""
    w64 = constants(plan_lib)["window_words"] * 64
    groups, m = 3 * w64 + 77, 5
    n = groups + 6710
    rng = np.random.default_rng(8)
    perm = ((np.arange(groups, dtype=np.uint64) * np.uint64(104729)) % np.uint64(groups)).astype(np.uint32)
    assert np.unique(perm).size == groups                                # (104729 is prime and does not divide G)
    group_of = np.concatenate([perm, rng.integers(0, groups, n - groups).astype(np.uint32)])
    p = plan(plan_lib, n, group_of, groups, m=m, tables=False)
    assert p["windows"] >= 3 and p["dst_words"] % p["window_words"] not in (0, p["window_words"] - 1)
    bits = (rng.random((m, n)) < 0.3).astype(np.uint8)
    check_collapse(bits, group_of, groups, "many-to-one")
    injective = group_of.copy()
    injective[groups:] = DROPPED
    src, dst, ext = source(bits), Raw(m=m, n=0, cap=1), Raw(m=m, n=0, cap=1)
    try:
        assert collapse(dst, src.ix, injective, groups) == 0, dst.L.bigsi_hip_last_error()
        assert ext.L.bigsi_hip_extract_columns(ext.ix, src.ix, ptr(pack_keep(injective != DROPPED))) == 0, ext.L.bigsi_hip_last_error()
        taken = np.unpackbits(ext.rows(row_bytes=(groups + 7) // 8), axis=1)[:, :groups]
        assert np.array_equal(taken, bits[:, :groups])
        reordered = np.zeros_like(taken)
        reordered[:, perm] = taken
        full = dst.rows()
        want = np.zeros_like(full)
        want[:, :(groups + 7) // 8] = np.packbits(reordered, axis=1)
        assert np.array_equal(full, want)
    finally:
        for r in (src, dst, ext):
            r.close()


def test_e_views_as_source_and_refusals():
    bits = ragged_bits(300, 200)
    label, group_of, groups = collapse_maps(200)[4]
    a, dst, other_m, other_h, full = source(bits), Raw(m=300, n=0, cap=1), Raw(m=301, n=0, cap=1), Raw(m=300, n=0, cap=1), Raw.from_bits(bits)
    L = a.L
    a.lib.check(L.bigsi_hip_set_num_hashes(other_h.ix, 2))
    view, dst_view = C.c_void_p(), C.c_void_p()
    a.lib.check(L.bigsi_hip_open_view(a.ix, C.byref(view)))
    a.lib.check(L.bigsi_hip_open_view(dst.ix, C.byref(dst_view)))
    bad = group_of.copy()
    bad[141] = groups + 5
    try:
        before = a.rows()
        for call, want, words in ((lambda: collapse(dst, None, group_of, groups), ERR_INVALID, ()),
                                  (lambda: L.bigsi_hip_collapse_columns_into(None, a.ix, ptr(group_of), groups), ERR_INVALID, ()),
                                  (lambda: L.bigsi_hip_collapse_columns_into(other_m.ix, a.ix, None, groups), ERR_INVALID, ()),
                                  (lambda: collapse(other_m, a.ix, group_of, groups), ERR_INVALID, ("301", "300")),
                                  (lambda: collapse(other_h, a.ix, group_of, groups), ERR_INVALID, ("2", "3")),
                                  (lambda: collapse(other_h, a.ix, group_of, 0), ERR_INVALID, ("0",)),
                                  (lambda: collapse(other_h, a.ix, group_of, 0xFFFFFFFF), ERR_INVALID, ("4294967295",)),
                                  (lambda: collapse(a, a.ix, group_of, groups), ERR_INVALID, ()),                          # dst == src
                                  (lambda: collapse(dst, dst_view, group_of, groups), ERR_INVALID, ("view",)),             # src a view of dst
                                  (lambda: L.bigsi_hip_collapse_columns_into(view, full.ix, ptr(group_of), groups), ERR_STATE, ("read-only",)),   # dst a view
                                  (lambda: collapse(dst, a.ix, group_of, groups), ERR_STATE, ("view",)),                   # dst an owner with a view open
                                  (lambda: collapse(full, a.ix, group_of, groups), ERR_STATE, ("200",))):                  # dst holds columns
            rc = call()
            msg = L.bigsi_hip_last_error().decode()
            assert rc == want and msg and all(w in msg for w in words), (rc, want, msg)
        a.lib.check(L.bigsi_hip_close(dst_view))
        dst_view = None
        rc = collapse(dst, a.ix, bad, groups)                                                                            # names the column and the value
        msg = L.bigsi_hip_last_error().decode()
        assert rc == ERR_INVALID and "141" in msg and str(groups + 5) in msg
        for r in (dst, other_m, other_h):          # a refused call left the destination empty
            assert r.info().num_cols == 0 and not r.rows().any()
        assert np.array_equal(full.rows(row_bytes=25), np.packbits(bits, axis=1)) and full.info().num_cols == 200
        assert np.array_equal(a.rows(), before) and a.info().num_cols == 200 == a.info(view).num_cols
        # a view AS THE SOURCE works
        assert collapse(dst, view, group_of, groups) == 0, L.bigsi_hip_last_error()
        got = dst.rows()
        assert np.array_equal(got, expected_rows(bits, group_of, groups, got.shape[1])) and dst.info().num_cols == groups
    finally:
        for v in (view, dst_view):
            if v is not None:
                a.lib.check(L.bigsi_hip_close(v))
        for r in (a, dst, other_m, other_h, full):
            r.close()


def test_f_an_ipc_handle_is_a_source_and_no_destination():
    """An index attached over hipIpc in a child process: collapsed from there into an index of the child's own, refused as destination."""
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
                "five = np.zeros(5, np.uint32)\n"
                "rc = [L.bigsi_hip_collapse_columns_into(dst, ix, g.ctypes.data_as(C.c_void_p), 7)]\n"
                "out = np.zeros((60, 128), np.uint8); ids = np.arange(60, dtype=np.uint64)\n"
                "_lib.check(L.bigsi_hip_get_rows(dst, ids.ctypes.data_as(C.c_void_p), 60, out.ctypes.data_as(C.c_void_p), 128))\n"
                "rc.append(L.bigsi_hip_collapse_columns_into(ix, own, five.ctypes.data_as(C.c_void_p), 1))\n"
                "print(rc[0], rc[1], out.tobytes().hex())\n"
                "for x in (ix, dst, own): _lib.check(L.bigsi_hip_close(x))\n") % (ROOT, handle.tobytes().hex())
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        rc0, rc1, rows = r.stdout.split()
        assert (int(rc0), int(rc1)) == (0, ERR_STATE)
        g = (np.arange(100) % 7).astype(np.uint32)
        g[::9] = DROPPED
        assert np.array_equal(np.frombuffer(bytes.fromhex(rows), np.uint8).reshape(60, 128), expected_rows(bits, g, 7, 128))
        assert np.array_equal(a.rows(row_bytes=13), np.packbits(bits, axis=1)) and a.info().num_cols == 100
    finally:
        a.close()


# --------------------------------------------------------------------------------------------- BIGSI level
K, M, H, N_SAMPLES = 11, 4099, 3, 70


def config(d, tag):
    return {"storage-engine": "hip-hbm", "k": K, "m": M, "h": H, "storage-config": {"name": "col%s%d" % (tag, next(_counter)), "filename": str(d / ("%s.hbm" % tag))}}


def state_of(b):
    """(every host-side record, every row at the full stride) of an index."""
    st = b.storage
    rows = st.res.get_rows(np.arange(M, dtype=np.uint64), int(st.res.info().row_stride_bytes))
    return {k: st[k] for k in st.record_keys()}, np.asarray(rows)


def searches(b, queries):
    return [b.search(queries[0]), b.search(queries[1], 0.4), b.search(queries[0], score=True), b.search(queries[1], 0.4, score=True)]


def union_filter(filters, members):
    """The numpy-OR of the members' Bloom filters: the filter of the union of their k-mer sets."""
    from bigsi_amd.bitrow import BitRow
    acc = np.zeros((M + 7) // 8, np.uint8)
    for n in members:
        acc |= np.frombuffer(filters[n].tobytes(), np.uint8)
    return BitRow.frombytes(acc.tobytes(), M)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """70 samples (the colours cross a 64-column word), each a mutated copy of one base sequence so that a query has many partial
    hits; their Bloom filters from BIGSI.bloom are what a fresh build is made of."""
    from bigsi_amd import BIGSI
    from bigsi_amd.utils import seq_to_kmers
    rng = np.random.default_rng(78)
    base = rand_seq(rng, 240)
    seqs = {}
    for c in range(N_SAMPLES):
        cut = int(rng.integers(60, 200))
        seqs["s%d" % c] = base[:cut] + rand_seq(rng, 240 - cut)
    d = tmp_path_factory.mktemp("collapse")
    cfg = config(d, "main")
    b = BIGSI.build_from_sequences(cfg, {n: [s] for n, s in seqs.items()})
    filters = {n: BIGSI.bloom(cfg, list(seq_to_kmers(s, K))) for n, s in seqs.items()}
    made = [b]
    yield {"b": b, "cfg": cfg, "dir": d, "seqs": seqs, "filters": filters, "queries": [base[:100], base[:200]], "made": made}
    for x in made:
        x.delete()


def world_groups():
    """Five groups over 47 of the 70 samples, named in an order that is not the colour order; 23 samples stay unlisted."""
    return {"late": ["s%d" % c for c in range(60, 70)], "odd": ["s%d" % c for c in range(1, 40, 2)], "single": ["s0"],
            "span": ["s58", "s2", "s59", "s4"], "even": ["s%d" % c for c in range(6, 30, 2)]}


def test_g_collapse_equals_a_fresh_build_of_the_or_ed_filters(world):
    from bigsi_amd import BIGSI
    from bigsi_amd.collapse import collapse_plan
    b, d, q = world["b"], world["dir"], world["queries"]
    groups = world_groups()
    before = state_of(b)
    new = b.collapse(config(d, "grouped"), groups)
    names = list(groups)
    fresh = BIGSI.build(config(d, "groupedfresh"), [union_filter(world["filters"], groups[g]) for g in names], names)
    world["made"] += [new, fresh]
    assert new.num_samples == len(names) and [new.colour_to_sample(c) for c in range(len(names))] == names
    (kv1, rows1), (kv2, rows2) = state_of(new), state_of(fresh)
    assert kv1 == kv2 and np.array_equal(rows1, rows2)
    got = searches(new, q)
    assert got == searches(fresh, q) and len(got[0]) > 0 and len(got[1]) > 1
    # the source is as it was, and the membership is what the plan says
    after = state_of(b)
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and b.num_samples == N_SAMPLES
    _, out, members = collapse_plan(["s%d" % c for c in range(N_SAMPLES)], groups)
    assert out == names and [sorted(m) for m in members] == [sorted(groups[g]) for g in names]
    # no false negatives: every exact hit of a member in the source is a hit of its group
    group_of_sample = {s: g for g, ms in groups.items() for s in ms}
    for query in (q[0], world["seqs"]["s61"][:80], world["seqs"]["s7"][100:180]):
        hit_groups = {r["sample_name"] for r in new.search(query)}
        hits = [r["sample_name"] for r in b.search(query)]
        assert hits and all(group_of_sample[s] in hit_groups for s in hits if s in group_of_sample)


def test_h_keep_others_and_deleted_samples(world):
    from bigsi_amd import BIGSI
    b, d = world["b"], world["dir"]
    groups = world_groups()
    with pytest.raises(ValueError):
        b.collapse(dict(config(d, "never"), m=M + 1), groups)
    for bad, err in (({"A": ["nobody"]}, KeyError), ({"A": ["s1"], "B": ["s1"]}, ValueError), ({}, ValueError)):
        with pytest.raises(err):
            b.collapse(config(d, "never"), bad)
    b.delete_sample("s3")          # a member of "odd"...
    b.delete_sample("s41")         # ... and an unlisted sample
    with pytest.raises(KeyError):
        b.collapse(config(d, "never"), groups)                            # a deleted name
    groups["odd"].remove("s3")
    new = b.collapse(config(d, "others"), groups, keep_others=True)
    world["made"].append(new)
    listed = {s for ms in groups.values() for s in ms}
    rest = ["s%d" % c for c in range(N_SAMPLES) if "s%d" % c not in listed and c not in (3, 41)]
    names = list(groups) + rest
    assert [new.colour_to_sample(c) for c in range(new.num_samples)] == names and new.num_samples == len(names) == 5 + 22
    members = [groups[g] for g in groups] + [[s] for s in rest]
    fresh = BIGSI.build(config(d, "othersfresh"), [union_filter(world["filters"], ms) for ms in members], names)
    world["made"].append(fresh)
    (kv1, rows1), (kv2, rows2) = state_of(new), state_of(fresh)
    assert kv1 == kv2 and np.array_equal(rows1, rows2)
    assert searches(new, world["queries"]) == searches(fresh, world["queries"])


def test_i_groups_are_refused(tmp_path):
    from bigsi_amd import BIGSI
    from bigsi_amd._lib import BigsiHipError
    rng = np.random.default_rng(10)
    cfg = config(tmp_path, "grp")
    cfg["storage-config"].update(devices=[0, 0], max_cols=8)
    del cfg["storage-config"]["filename"]
    b = BIGSI.build_from_sequences(cfg, {"g%d" % c: [rand_seq(rng, 60)] for c in range(6)})
    try:
        for call in (lambda: b.collapse(config(tmp_path, "never"), {"A": ["g1", "g2"]}),
                     lambda: b.storage.collapse_columns_into(b.storage, np.zeros(6, np.uint32), 1)):
            with pytest.raises(BigsiHipError) as e:
                call()
            assert e.value.code == ERR_STATE
        assert b.num_samples == 6
    finally:
        b.delete()


def test_j_cli_collapse_then_search(tmp_path, capsys):
    """`python -m bigsi_amd collapse` in a process of its own on an index's snapshot, then a `search` under the new config (through the
    same main(), on the snapshot the child left) that sees the groups."""
    from bigsi_amd import BIGSI
    from bigsi_amd.__main__ import main
    from bigsi_amd.storage.hip_hbm import HipHbmStorage
    rng = np.random.default_rng(12)
    cfg, to = config(tmp_path, "cli"), config(tmp_path, "clito")
    seqs = {"c%d" % c: [rand_seq(rng, 90)] for c in range(7)}
    b = BIGSI.build_from_sequences(cfg, seqs)
    b.delete_sample("c4")
    b.storage.sync()
    HipHbmStorage.drop(cfg["storage-config"]["name"])                     # (the snapshot is what the child process sees)
    cf, tf, gf = tmp_path / "config.yaml", tmp_path / "to.yaml", tmp_path / "groups.tsv"
    cf.write_text(yaml.safe_dump(cfg))
    tf.write_text(yaml.safe_dump(to))
    gf.write_text("c6\tB\nc0\tA\nc2\tB\n\nc5\tA\n")
    r = subprocess.run([sys.executable, "-m", "bigsi_amd", "collapse", str(tf), "--groups", str(gf), "--config", str(cf)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    try:
        assert json.loads(r.stdout) == {"result": "collapsed 4 of 6 samples from %s into 2 groups in %s." % (cf, tf), "groups": 2, "samples_in": 6,
                                        "samples_dropped": 2, "num_samples": 2, "members": {"B": ["c2", "c6"], "A": ["c0", "c5"]}}
        for sample, group in (("c5", "A"), ("c2", "B")):
            capsys.readouterr()
            assert main(["search", seqs[sample][0][:50], "--config", str(tf)]) == 0
            assert [x["sample_name"] for x in json.loads(capsys.readouterr().out)["results"]] == [group]
        capsys.readouterr()
        assert main(["search", seqs["c1"][0][:50], "--config", str(tf)]) == 0          # a dropped sample is in no group
        assert json.loads(capsys.readouterr().out)["results"] == []
        new = BIGSI(to)
        assert [new.colour_to_sample(c) for c in range(new.num_samples)] == ["B", "A"]
    finally:
        for c in (to, cfg):
            if os.path.exists(c["storage-config"]["filename"]):
                BIGSI(c).delete()
