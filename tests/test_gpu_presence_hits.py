"""K5 at scale -- bigsi_hip_batch_presence_hits and its group twin (k_presence_bits, k_presence_pieces, k_presence_expand<true> /
<false>, k_presence_expand_listed, and the pair / wavefront lists presence_begin builds on the host) -- against the plain
reference of tests/presence_reference.py, EVERY string of EVERY hit: at the wavefront cut of the pair list (64 pairs), the 32-rank
tiles of the presence bits, every `pieces` geometry of the expand kernel and every branch of its lane arithmetic, with the
batch's workspace reused across calls, through the packed route (K6, score_hits) and the single-sequence kernel as well, over a
three-shard group, and the contract of the call as include/bigsi_hip.h states it.  Needs a real MI355X: `pytest -m gpu`."""
import itertools

import numpy as np
import pytest

import presence_reference as pref

pytestmark = pytest.mark.gpu

K, M = pref.K, 65537
_counter = itertools.count()


# ------------------------------------------------------------------------------------------------------------------ set-up
def open_storage(n_cols, h, devices=None, m=M):
    from bigsi_amd.storage import get_storage
    sc = {"name": "k5_%d" % next(_counter), "max_cols": n_cols}
    if devices:
        sc["devices"] = devices
    st = get_storage({"storage-engine": "hip-hbm", "storage-config": sc, "k": K, "m": m, "h": h})
    st.delete_all()
    for key, v in (("number_of_rows", m), ("number_of_cols", n_cols), ("ksi:bloomfilter_size", m), ("ksi:num_hashes", h)):
        st.set_integer(key, v)
    return st


class GroupOracle(object):
    """The shards' oracles side by side: shard i holds the global colours [i * shard_cols, ...), whole bytes each."""

    def __init__(self, st, h, seed):
        from oracle.ref_model import SynthOracle
        inf = st.res.info()
        self.sc, self.total, self.k = int(inf.shard_cols), int(inf.num_cols), K
        assert self.sc % 8 == 0
        self.orcs = [SynthOracle(seed, i, M, max(0, min(self.sc, self.total - i * self.sc)), h, K, 1) for i in range(int(inf.n_shards))]

    def insert_kmers(self, col, seq):
        self.orcs[col // self.sc].insert_kmers(col % self.sc, seq)

    def per_kmer_rows(self, seq):
        parts = [o.per_kmer_rows(seq) for o in self.orcs]
        rows = np.zeros((len(parts[0][1]), len(self.orcs) * self.sc // 8), np.uint8)
        for i, (_, _, r) in enumerate(parts):
            rows[:, i * self.sc // 8: i * self.sc // 8 + r.shape[1]] = r
        return parts[0][0], parts[0][1], rows


class Ref(object):
    """The index on the device (over `devices`: a group) and its oracle, filled alike; per_kmer_rows of every query computed once."""

    def __init__(self, n_cols, h, seed, devices=None):
        from oracle.ref_model import SynthOracle
        self.n_cols, self.h = n_cols, h
        self.st = open_storage(n_cols, h, devices=devices)
        self.st.fill_synthetic(seed, 0, 1)                  # (a group: shard i as (seed, i))
        self.orc = GroupOracle(self.st, h, seed) if devices else SynthOracle(seed, 0, M, n_cols, h, K, 1)
        self._rows = {}

    def plant(self, col, seq):
        assert not self._rows
        self.st.insert_kmers(int(col), [seq], K)
        self.orc.insert_kmers(int(col), seq)

    def matrix(self, seq, colours):
        """uint8[len(colours), n]: the expected characters."""
        if seq not in self._rows:
            self._rows[seq] = self.orc.per_kmer_rows(seq)[2]
        return pref.presence_matrix(self.orc, seq, colours, self._rows[seq])

    def close(self):
        self.st.delete_all()


def flatten(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in lists])
    colours = np.concatenate([np.asarray(c, dtype=np.uint32) for c in lists]) if lists else np.zeros(0, np.uint32)
    return off, np.ascontiguousarray(colours, dtype=np.uint32)


def assert_chars(got, want, what):
    if not np.array_equal(got, want):
        t, i = [int(x[0]) for x in np.nonzero(got != want)]
        raise AssertionError("%r: hit %d of the sequence, position %d (piece %d): %r, want %r; %d characters differ in %d hits"
                             % (what, t, i, i >> 4, bytes(got[t, max(i - 8, 0):i + 8]), bytes(want[t, max(i - 8, 0):i + 8]),
                                int((got != want).sum()), int((got != want).any(axis=1).sum())))


def check_text(batch, seqs, lists, ref, what):
    """presence_hits for lists[i] = the colours of sequence i, every character of every hit against the reference.  Returns the
    expected matrices, one per sequence."""
    off, colours = flatten(lists)
    nk, nu, _ = batch.unique()
    blob, starts, lens = batch.presence_hits(off, colours, nk)
    assert not (starts % 16).any()
    wants = []
    for i, s in enumerate(seqs):
        n, lo, hi = max(len(s) - K + 1, 0), int(off[i]), int(off[i + 1])
        assert nk[i] == n and (lens[lo:hi] == n).all() and nu[i] == (int(pref.position_map(s, K).max()) + 1 if n else 0)
        want = ref.matrix(s, lists[i])
        assert want.shape == (hi - lo, n)
        assert_chars(blob[starts[lo:hi, None] + np.arange(n)[None, :]], want, (what, "text", i))
        wants.append(want)
    return wants


def check_packed(batch, seqs, lists, wants, what):
    """K6's packed bits for the same lists: unpack_presence(score_hits(...)) must be the same characters."""
    from bigsi_amd.scoring import unpack_presence
    off, colours = flatten(lists)
    nk = batch.unique()[0]
    rec, bits, boff = batch.score_hits(off, colours, None, nk)
    text = np.frombuffer(unpack_presence(bits, boff).encode("ascii"), np.uint8)
    assert not (boff % 8).any() and int(boff[-1]) * 8 == text.size
    for i, s in enumerate(seqs):
        n, lo, hi = max(len(s) - K + 1, 0), int(off[i]), int(off[i + 1])
        if n and hi > lo:
            assert (rec["num_kmers"][lo:hi] == n).all()
            assert_chars(text[8 * boff[lo:hi, None].astype(np.int64) + np.arange(n)[None, :]], wants[i], (what, "packed", i))


def check_single(batch, seqs, lists, wants, what):
    """The single-sequence kernel (bigsi_hip_batch_presence), one sequence at a time."""
    for i, s in enumerate(seqs):
        n = max(len(s) - K + 1, 0)
        if n and len(lists[i]):
            got = batch.presence(i, lists[i], n)
            assert got == [r.tobytes().decode("ascii") for r in wants[i]], (what, "single", i)


def check_all_routes(batch, seqs, lists, ref, what):
    wants = check_text(batch, seqs, lists, ref, what)
    check_packed(batch, seqs, lists, wants, what)
    check_single(batch, seqs, lists, wants, what)
    return wants


# ------------------------------------------------------------------------------------------- a. wave and tile edges, every h
@pytest.mark.parametrize("n_cols", [8193, 16385])
@pytest.mark.parametrize("h", [1, 2, 3, 4, 5, 6, 8])
def test_wave_and_tile_edges(h, n_cols):
    """65 and 129 pairs of 128 columns per all-column query: the pair list is cut into wavefronts of 64 + 1 and 64 + 64 + 1; all
    columns also cross every 32-rank tile of the presence bits.  h = 1 .. 5 are the templated k_presence_bits, 6 and 8 the
    runtime-h one.  Lengths around the 16-position piece and the 64-position word; hit lists in any order; a sequence without
    k-mers whose hits come back as empty strings.  The text route, the packed route and the single-sequence kernel must all
    give the reference's characters for every hit."""
    rng = np.random.default_rng(1000 * h + n_cols)
    lens = {"n1": 1, "n15": 15, "n16": 16, "n17": 17, "n63": 63, "n64": 64, "n65": 65}
    q = {name: pref.rand_seq(rng, n + K - 1) for name, n in lens.items()}
    q["n300"] = pref.repeat_query(rng, 100, 130)              # 300 positions with a repeat: listed pieces and shifted runs too
    q["short"] = pref.rand_seq(rng, K - 1)
    assert len(q["n300"]) - K + 1 == 300
    ref = Ref(n_cols, h, seed=40 + h)
    edge = list(dict.fromkeys([0, 63, 64, 127, 128, 8191, 8192, n_cols - 1]))      # (8193 columns: the last one is 8192)
    for col, s in ((0, q["n300"][:200]), (8192, q["n300"][50:]), (n_cols - 1, q["n300"]), (63, q["n65"]), (8191, q["n65"][:60]), (64, q["n64"]),
                   (127, q["n63"][:50]), (4097, q["n63"]), (128, q["n17"]), (8191, q["n17"]), (n_cols - 1, q["n15"]), (0, q["n1"]), (5000, q["n16"])):
        ref.plant(col, s)
    order = ["n1", "n300", "n64", "short", "n63", "n17", "n16", "n65", "n15"]
    lists = {"n1": rng.permutation(n_cols)[:5],                # (5 hits first: the groups of four ranks straddle sequences from here on)
             "n300": np.arange(n_cols), "n65": np.arange(n_cols),
             "n64": np.arange(0, n_cols, 3)[::-1],             # reversed
             "n63": rng.permutation(n_cols)[:1000],
             "n17": np.array(edge), "n15": np.array(edge)[rng.permutation(len(edge))],
             "n16": np.zeros(0, int),
             "short": np.array([3, 0, n_cols - 1])}
    seqs, cl = [q[name] for name in order], [lists[name] for name in order]
    batch = ref.st.new_batch(seqs, K)
    batch.run(1.0)
    wants = check_all_routes(batch, seqs, cl, ref, (h, n_cols))
    # the inputs are not trivial: the planted columns are all ones, the others mixed (h <= 4) or sparse
    w300 = wants[order.index("n300")]
    assert (w300[n_cols - 1] == ord("1")).all() and (w300[0, :170] == ord("1")).all() and (w300 == ord("0")).any()
    assert (w300 == ord("1")).any(axis=1).sum() > (n_cols // 2 if h <= 3 else 20)
    batch.close()
    ref.close()


# ---------------------------------------------------------------------------------------------- b. long queries with repeats
@pytest.fixture(scope="module")
def ref200():
    """200 columns, h = 3, pieces of every query of pref.long_queries() planted in a few columns each."""
    ref = Ref(200, 3, seed=17)
    rng = np.random.default_rng(200)
    for name, s in pref.long_queries().items():
        if name == "nohits":
            continue
        for col in rng.permutation(200)[:4]:
            lo = int(rng.integers(0, max(len(s) - K, 1)))
            ref.plant(col, s[lo:lo + int(rng.integers(K, len(s) + 1))])
        ref.plant(int(rng.integers(0, 200)), s)
    yield ref
    ref.close()


# batch -> (queries, pieces per hit, classes its hit-bearing queries must reach between them); "nohits" never gets a hit
FULL = {"listed", "lo_shuffle", "lo_global", "hi_unused", "hi_shuffle", "hi_global", "delta_eq_sub_plus_1", "delta_eq_sub_pos", "r0_lo_global",
        "delta_pos", "tail"}
ONE_WAVE = {"listed", "lo_shuffle", "hi_unused", "hi_shuffle", "delta_pos"}
LONG_BATCHES = {
    "true256": (["rep128", "rep256", "rep32", "ac500", "ac330", "read61"], 256, FULL),
    "false32": (["rep32", "ac330", "read61", "nohits"], 32, ONE_WAVE | {"tail"}),
    "g1": (["run16", "per16", "run9", "run1", "nohits"], 1, {"listed", "lo_shuffle", "hi_unused", "tail"}),
    "g2": (["per32", "run17", "run16", "nohits"], 2, {"listed", "lo_shuffle", "hi_shuffle", "hi_unused", "delta_eq_sub_pos", "tail"}),
    "g4": (["rep64", "rep56", "per32", "nohits"], 4, ONE_WAVE | {"tail"}),
    "p63": (["rep1008", "rep32", "nohits"], 64, ONE_WAVE | {"delta_eq_sub_pos", "tail"}),
    "p64": (["rep1024", "rep1008", "nohits"], 64, ONE_WAVE | {"delta_eq_sub_pos"}),
    # 20 unique k-mers in the only hit-bearing query: 2 chunks of presence bits under 32 / 128 pieces per hit
    "clamp32": (["per300", "nohits"], 32, ONE_WAVE | {"delta_eq_sub_pos", "tail"}),
    "clamp128": (["nohits", "per1070"], 128, ONE_WAVE | {"lo_global", "hi_global", "tail_listed"}),
}


def long_batch(name):
    qs = pref.long_queries()
    names, pieces, classes = LONG_BATCHES[name]
    bearing = [x for x in names if x != "nohits"]
    assert pref.pieces_for(max(len(qs[x]) - K + 1 for x in bearing)) == pieces
    reached = set()
    for x in bearing:
        reached |= set(pref.class_names(pref.position_map(qs[x], K), pieces))
    assert classes <= reached, (name, classes - reached)
    return names, [qs[x] for x in names]


@pytest.mark.parametrize("name", sorted(LONG_BATCHES))
def test_long_queries_with_repeats(ref200, name):
    """Every `pieces` geometry of k_presence_expand (G = 1, 2, 4, 32 in <false>; 64, 128 and 256 pieces in <true>, 63 pieces rounded
    up to 64 beside exactly 64) with queries whose pieces are runs that start in the thread's own chunk, in a chunk held by a lane
    of the same wavefront, at the edge of it, or in another wavefront, and listed pieces; `pieces` comes from the hit-bearing
    sequences, so a longer sequence without hits rides along.  The branch classes are asserted on the CPU before the device runs."""
    names, seqs = long_batch(name)
    rng = np.random.default_rng(len(name) + LONG_BATCHES[name][1])
    lists = [np.zeros(0, int) if x == "nohits" else rng.permutation(200)[:200 - 3 * i - 1] for i, x in enumerate(names)]
    batch = ref200.st.new_batch(seqs, K)
    batch.run(1.0)
    wants = check_all_routes(batch, seqs, lists, ref200, name)
    assert all((w == ord("1")).any() and (w == ord("0")).any() for w, x in zip(wants, names) if x != "nohits")      # (mixed strings)
    batch.close()


# ------------------------------------------------------------------------------------------------------ c. workspace reuse
def test_workspace_reuse(ref200):
    """One batch object through everything that keeps state between calls: the presence bits (chunks above a sequence's unique
    count are never rewritten), the piece marks (once per run, again when their buffer moves), the staging buffers."""
    qs = pref.long_queries()
    rng = np.random.default_rng(5)
    names = ["rep32", "ac330", "read61", "run17", "rep56"]
    seqs = [qs[x] for x in names]
    none = np.zeros(0, int)
    batch = ref200.st.new_batch(seqs, K)
    batch.run(1.0)
    check_text(batch, seqs, [np.arange(200)] * 5, ref200, "all columns")
    check_text(batch, seqs, [none, none, np.array([199, 0, 64]), none, none], ref200, "three columns of a short one")      # 2 chunks, 2 pieces now
    check_text(batch, seqs, [np.array([5, 128, 127]), none, none, none, none], ref200, "three columns of a long one")
    batch.run(0.5)
    check_text(batch, seqs, [rng.permutation(200)[:50 + i] for i in range(5)], ref200, "after another run")
    # both routes on one run: the marks are computed once, the presence bits rewritten by every call
    a, b, c = ([rng.permutation(200)[:n0 + 7 * i] for i in range(5)] for n0 in (9, 60, 31))
    wa = check_text(batch, seqs, a, ref200, "interleaved 1")
    check_packed(batch, seqs, b, [ref200.matrix(s, l) for s, l in zip(seqs, b)], "interleaved 2")
    check_text(batch, seqs, c, ref200, "interleaved 3")
    check_packed(batch, seqs, a, wa, "interleaved 4")
    check_text(batch, seqs, b, ref200, "interleaved 5")
    # shorter sequences in the same buffers
    seqs = [qs[x] for x in ("run9", "per16", "read61")]
    batch.reload(seqs)
    batch.run(1.0)
    check_all_routes(batch, seqs, [np.arange(200)[::-1], rng.permutation(200)[:77], np.arange(200)], ref200, "reloaded shorter")
    # longer ones: every buffer regrows, the marks move
    seqs = [qs[x] for x in ("rep256", "ac500", "rep128", "rep1008")]
    batch.reload(seqs)
    batch.run(1.0)
    check_all_routes(batch, seqs, [rng.permutation(200)[:150], np.arange(200), rng.permutation(200)[:33], none], ref200, "reloaded longer")
    check_text(batch, seqs, [none, none, none, np.array([7, 3])], ref200, "after the long ones")
    batch.close()


# ------------------------------------------------------------------------------------------------------------------ e. group
@pytest.fixture(scope="module")
def group500():
    """500 columns over devices [0, 0, 0]: shards of 192 + 192 + 116 columns (whole 64-bit words by construction), so the cuts at
    192 and 384 fall inside the 128-column pair [128, 256) and on a pair edge, and the index ends inside a word.  Beside it a
    single index holding the same rows."""
    n_cols, h, seed = 500, 3, 23
    ref = Ref(n_cols, h, seed, devices=[0, 0, 0])
    inf = ref.st.res.info()
    assert (int(inf.n_shards), int(inf.shard_cols), int(inf.num_cols)) == (3, 192, 500)
    qs = pref.long_queries()
    for name, cols in (("rep32", (0, 191, 192, 300)), ("ac330", (193, 383, 384)), ("read61", (127, 128, 499)), ("run17", (255, 256, 498))):
        for j, col in enumerate(cols):
            ref.plant(col, qs[name][: len(qs[name]) - 20 * j])
    single = open_storage(n_cols, h)
    single.set_rows_packed(0, ref.st.get_rows_packed(np.arange(M, dtype=np.uint64), (n_cols + 7) // 8))
    yield ref, single
    single.delete_all()
    ref.close()


def group_case(rng):
    qs = pref.long_queries()
    seqs = [qs["read61"], qs["rep32"], qs["ac330"], qs["run17"], "ACGT", qs["run9"]]
    lists = [np.array([191, 0, 192, 499, 383, 193, 384, 127, 256, 128, 255]),      # shards 0 0 1 2 1 1 2 0 1 0 1
             rng.permutation(500), np.arange(500)[::-1], rng.permutation(500)[:99], np.array([400, 5, 200]), np.zeros(0, int)]
    return seqs, lists


def test_group_equals_single_index_and_reference(group500):
    """Each shard produces the strings of the hits it owns and the host puts them in the caller's order: colour lists that
    interleave the shards in arbitrary order, every string against the reference and against a single index with the same rows."""
    ref, single = group500
    seqs, lists = group_case(np.random.default_rng(9))
    gb = ref.st.new_batch(seqs, K)
    gb.run(1.0)
    check_all_routes(gb, seqs, lists, ref, "group")
    sb = single.new_batch(seqs, K)
    sb.run(1.0)
    # the single index: the same offsets, and character for character the group's strings (the padding between them is not compared)
    off, colours = flatten(lists)
    nk = sb.unique()[0]
    (gblob, gstart, glen), (sblob, sstart, slen) = gb.presence_hits(off, colours, nk), sb.presence_hits(off, colours, nk)
    assert np.array_equal(gstart, sstart) and np.array_equal(glen, slen)
    for t in range(len(sstart)):
        assert np.array_equal(gblob[gstart[t]:gstart[t] + glen[t]], sblob[sstart[t]:sstart[t] + slen[t]]), t
    check_all_routes(sb, seqs, lists, ref, "single index")
    gb.close()
    sb.close()


# -------------------------------------------------------------------------------------------------- f. contract of the call
def raw_call(batch, off, colours, capacity, n_hits):
    """The C call itself: (return code, out, string_offsets), out preset to 0xEE."""
    from bigsi_amd import _lib
    out = np.full(max(int(capacity), 16), 0xEE, np.uint8)
    soff = np.full(n_hits + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    rc = batch._fn("presence_hits")(batch.b, _lib.ptr(off), None if colours is None else _lib.ptr(colours), _lib.ptr(out), int(capacity), _lib.ptr(soff))
    return rc, out, soff


@pytest.mark.parametrize("which", ["single", "group"])
def test_contract_of_the_call(ref200, group500, which):
    """include/bigsi_hip.h on bigsi_hip_batch_presence_hits: offsets are multiples of 16 and the last one is the bytes needed;
    too small a buffer -> ERR_CAPACITY with the offsets filled, and the retry succeeds; hit_offsets need not start at 0; no hits;
    a colour twice -> ERR_INVALID; a colour >= num_cols -> ERR_RANGE; before run() -> ERR_STATE.  (The padding between strings is
    unspecified and not looked at.)"""
    from bigsi_amd import _lib
    ref = ref200 if which == "single" else group500[0]
    n_cols = ref.n_cols
    qs = pref.long_queries()
    seqs = [qs["rep32"], "ACGT", qs["read61"], qs["run17"], qs["run16"]]
    ns = [max(len(s) - K + 1, 0) for s in seqs]
    rng = np.random.default_rng(3)
    lists = [rng.permutation(n_cols)[:37], np.array([1, 0]), np.array([n_cols - 1, 0, 64, 63]), np.zeros(0, int), rng.permutation(n_cols)[:9]]
    off, colours = flatten(lists)
    n_hits = int(off[-1])
    batch = ref.st.new_batch(seqs, K)
    rc, _, _ = raw_call(batch, off, colours, 1 << 20, n_hits)
    assert rc == _lib.ERR_STATE
    batch.run(1.0)
    per_hit = np.repeat([(n + 15) // 16 * 16 for n in ns], [len(c) for c in lists])
    need = int(per_hit.sum())
    want_soff = np.concatenate([[0], np.cumsum(per_hit)]).astype(np.uint64)

    def strings_ok(out, soff, base=0):
        for i, s in enumerate(seqs):
            lo, hi = int(off[i]) - base, int(off[i + 1]) - base
            got = out[soff[lo:hi, None].astype(np.int64) + np.arange(ns[i])[None, :]]
            assert_chars(got, ref.matrix(s, lists[i]), (which, i))

    rc, out, soff = raw_call(batch, off, colours, need, n_hits)
    assert rc == _lib.OK and np.array_equal(soff, want_soff) and not (soff % 16).any() and int(soff[n_hits]) == need
    strings_ok(out, soff)
    rc, out, soff = raw_call(batch, off, colours, need // 2, n_hits)
    assert rc == _lib.ERR_CAPACITY and np.array_equal(soff, want_soff)
    rc, out, soff = raw_call(batch, off, colours, need - 1, n_hits)
    assert rc == _lib.ERR_CAPACITY and np.array_equal(soff, want_soff)
    rc, out, soff = raw_call(batch, off, colours, int(soff[n_hits]), n_hits)
    assert rc == _lib.OK and np.array_equal(soff, want_soff)
    strings_ok(out, soff)
    # a sliced caller: hit_offsets[0] > 0, colours indexed by the offsets as they are; what lies before is not read
    base = 6
    off2 = off + np.uint64(base)
    colours2 = np.concatenate([np.full(base, 0xFFFFFFFF, np.uint32), colours])
    rc, out, soff = raw_call(batch, off2, colours2, need, n_hits)
    assert rc == _lib.OK and np.array_equal(soff, want_soff)
    strings_ok(out, soff)
    # no hits at all, with and without a colour array
    zero = np.zeros(len(seqs) + 1, np.uint64)
    for col in (None, colours):
        rc, out, soff = raw_call(batch, zero, col, 0, 0)
        assert rc == _lib.OK and soff[0] == 0
    rc, out, soff = raw_call(batch, zero + np.uint64(4), colours, 0, 0)
    assert rc == _lib.OK and soff[0] == 0
    # hits only for the sequence without k-mers: empty strings, nothing needed
    only = np.array([0, 0, 2, 2, 2, 2], np.uint64)
    rc, out, soff = raw_call(batch, only, np.array([1, 0], np.uint32), 0, 2)
    assert rc == _lib.OK and soff.tolist() == [0, 0, 0]
    # a colour twice in one sequence (not adjacent); the same colour in two sequences is fine
    dup = [np.array([5, 9, 5]), np.zeros(0, int), np.array([5]), np.zeros(0, int), np.zeros(0, int)]
    rc, _, _ = raw_call(batch, *flatten(dup), 1 << 16, 4)
    assert rc == _lib.ERR_INVALID
    dup[0] = np.array([5, 9, 6])
    rc, out, soff = raw_call(batch, *flatten(dup), 1 << 16, 4)
    assert rc == _lib.OK
    assert_chars(out[int(soff[3]) + np.arange(ns[2])][None, :], ref.matrix(seqs[2], [5]), (which, "same colour in two sequences"))
    for bad in (n_cols, 0xFFFFFFFF):
        rng_list = [np.array([0, bad, 1], np.uint32)] + [np.zeros(0, np.uint32)] * 4
        rc, _, _ = raw_call(batch, *flatten(rng_list), 1 << 16, 3)
        assert rc == _lib.ERR_RANGE
    # after the refused calls the batch still answers
    rc, out, soff = raw_call(batch, off, colours, need, n_hits)
    assert rc == _lib.OK
    strings_ok(out, soff)
    batch.close()
