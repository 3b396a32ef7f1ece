"""Ranked top-N search, host side (no GPU): argument checks of `limit` / --limit, the new entry points of the C ABI, and a numpy
model of the ordering rule a limited search cuts by, pinned to the reference's own results (golden G3)."""
import argparse

import numpy as np
import pytest

from conftest import load_golden, unjson


def test_check_limit():
    from bigsi_amd.graph.bigsi import check_limit
    assert check_limit(None) is None
    assert check_limit(1) == 1 and check_limit(10 ** 12) == 10 ** 12 and check_limit(np.int64(5)) == 5
    for bad in (True, False, 2.0, "3", 1.5):
        with pytest.raises(TypeError):
            check_limit(bad)
    for bad in (0, -1, -(10 ** 9)):
        with pytest.raises(ValueError):
            check_limit(bad)


def test_bulk_search_rejects_a_bad_limit_before_any_device_work():
    from bigsi_amd.frontend import bulk_search
    with pytest.raises(ValueError):
        bulk_search(None, "no-such.fasta", limit=0)
    with pytest.raises(TypeError):
        bulk_search(None, "no-such.fasta", limit=True)


def test_cli_limit_parsing(capsys):
    from bigsi_amd.__main__ import main, positive_int
    assert positive_int("3") == 3
    for bad in ("0", "-2", "2.5", "x"):
        with pytest.raises(argparse.ArgumentTypeError):
            positive_int(bad)
    for cmd in (["search", "ACGT"], ["bulk_search", "q.fasta"], ["bulk_search", "q.fasta", "--stream"]):
        with pytest.raises(SystemExit) as e:
            main(cmd + ["--limit", "0"])
        assert e.value.code == 2
        with pytest.raises(SystemExit) as e:
            main(cmd + ["--limit", "3", "--sharded"])          # refused before any config is read or device opened
        assert e.value.code == 2
        assert "--limit is not available with --sharded" in capsys.readouterr().err


def test_new_entry_points_resolve():
    from bigsi_amd import _lib
    L = _lib.lib()
    for name in ("bigsi_hip_batch_set_limit", "bigsi_hip_search_stream_ranked", "bigsi_hip_group_batch_set_limit"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert _lib.limit_arg(10 ** 12) == 0xFFFFFFFF and _lib.limit_arg(7) == 7


def model_top_n(colours, counts, n, exact, excluded=()):
    """What a limited search keeps: excluded colours out, then the reference's order -- exact: ascending colour; thresholded:
    count descending, stable over ascending colours -- cut to n."""
    colours, counts = np.asarray(colours, np.int64), np.asarray(counts, np.int64)
    keep = ~np.isin(colours, np.asarray(excluded, np.int64))
    colours, counts = colours[keep], counts[keep]
    asc = np.argsort(colours, kind="stable")
    colours, counts = colours[asc], counts[asc]
    order = np.arange(colours.size) if exact else np.argsort(-counts, kind="stable")
    return colours[order[:n]].tolist()


def test_ordering_model_against_the_reference_results():
    """Every G3 search result list, shuffled and re-ranked by the model, cut to N == the reference's list cut to N -- ties included
    (G3's samples share many counts)."""
    g = load_golden("g3_search.json")
    names = list(g["samples"].keys())
    rng = np.random.default_rng(0)
    checked = ties = 0
    for s in g["searches"]:
        out = s["out"]
        if "raises" in out or not out["results"]:
            continue
        res = unjson(out["results"])
        cols = [names.index(r["sample_name"]) for r in res]
        cnts = [r["num_kmers_found"] for r in res]
        ties += len(set(cnts)) < len(cnts)
        perm = rng.permutation(len(cols))
        for n in (1, 2, 3, len(cols) + 1):
            got = model_top_n(np.asarray(cols)[perm], np.asarray(cnts)[perm], n, s["threshold"] == 1.0)
            assert got == cols[:n], (s["seq"], s["threshold"], n)
        checked += 1
    assert checked >= 20 and ties >= 5
    # deleted samples: the reference drops them after ordering, the model before the cut -- the same first N
    d = g["after_delete_a"]
    for s in d["searches"]:
        if "raises" in s["out"]:
            continue
        res = unjson(s["out"]["results"])
        assert all(r["sample_name"] != "a" for r in res)
