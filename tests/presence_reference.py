"""Reference for the presence strings of BIGSI.score (graph/bigsi.py:232-237) and a CPU mirror of the piece geometry of the
kernels that produce them on the device (k_presence_pieces / k_presence_expand, csrc/bigsi_kernels.hpp).  A plain module: nothing
here is collected, nothing here touches the device.  tests/test_presence_reference_host.py pins it to the CPU twin.

The unique k-mers of a query are its distinct k-mer STRINGS in first-occurrence order -- len(set(kmers)) of graph/bigsi.py:177-179,
`uniq` of oracle/ref_model.SynthOracle.per_kmer_rows, and what K1's dedupe compares (kmer_equal on the query's bytes): a k-mer and
its reverse complement, or its lower-case spelling, are two entries that happen to fetch the same rows."""
import numpy as np

from bigsi_amd.utils import seq_to_kmers


def position_map(seq, k):
    """int64[n]: for every k-mer position of seq the index of its k-mer among the query's unique k-mers, first-occurrence order
    (row j of per_kmer_rows(seq)[2] belongs to index j)."""
    first = {}
    return np.array([first.setdefault(km, len(first)) for km in seq_to_kmers(seq, k)], dtype=np.int64)


def presence_matrix(orc, seq, colours, rows=None):
    """uint8[len(colours), n] of ASCII '0' / '1': character i of row t is bit colours[t] of the AND of the h rows of the k-mer at
    position i, in the reference's bit order (column c = byte c >> 3 under mask 0x80 >> (c & 7)).  `rows` = per_kmer_rows(seq)[2]
    if the caller has it already."""
    colours = np.asarray(colours, dtype=np.int64)
    pm = position_map(seq, orc.k)
    if rows is None:
        rows = orc.per_kmer_rows(seq)[2]
    if pm.size == 0 or colours.size == 0:
        return np.zeros((colours.size, pm.size), np.uint8)
    assert rows.shape[0] == int(pm.max()) + 1
    bit = (rows[:, colours >> 3] & (0x80 >> (colours & 7)).astype(np.uint8)) != 0      # [unique k-mer, colour]
    return np.ascontiguousarray(bit[pm].T).view(np.uint8) + np.uint8(ord("0"))


def presence_strings(orc, seq, colours, rows=None):
    """The same as one str per colour."""
    mat = presence_matrix(orc, seq, colours, rows)
    return [r.tobytes().decode("ascii") for r in mat]


# ------------------------------------------------------------------------------------------- the queries of the GPU tests
# Built here so that tests/test_presence_reference_host.py can assert, without a device, that they still reach every branch.
K = 31


def rand_seq(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes().decode("ascii")


def repeat_query(rng, a, b):
    """A + A + B over random ACGT: positions 0 .. a - K are new, the K - 1 windows across the seam are new, then the windows of the
    second A repeat the first ones -- runs of consecutive unique indices that start a - K + 1 + K - 1 = a positions to the left, so
    `delta` is about a / 16 -- and B is new again, its unique indices a - K + 1 behind its positions (B starts with another letter
    than A, or the first window into B would repeat the first window across the seam and shift that by one)."""
    A, B = rand_seq(rng, a), rand_seq(rng, b)
    if B[0] == A[0]:
        B = "ACGT"["ACGT".index(B[0]) ^ 1] + B[1:]
    return A + A + B


def stutter_query(rng, n, unit=40):
    """About n characters over the alphabet AC in which one random unit of `unit` characters comes back every unit + 3 .. unit + 9
    characters: unit - K + 1 repeated windows between new ones each time, so a piece in three touches a repeat and is listed.  (A
    plain random AC string has no repeated 31-mer to speak of: 2^31 of them.)"""
    U, s = rand_seq(rng, unit, b"AC"), ""
    while len(s) + unit + 9 <= n:
        s += U + rand_seq(rng, int(rng.integers(3, 10)), b"AC")
    return s + rand_seq(rng, n - len(s), b"AC")


def long_queries():
    """name -> sequence: the queries of the long-query tests (section b of tests/test_gpu_presence_hits.py), K = 31."""
    rng = np.random.default_rng(3105)
    return {
        "rep128": repeat_query(rng, 600, 700),        # 1870 positions, 128 pieces: every branch but r == 0 across wavefronts
        "rep256": repeat_query(rng, 1054, 1500),      # 3578 positions, 256 pieces: adds r == 0 with the chunk in another wavefront
        "rep32": repeat_query(rng, 45, 300),          # 360 positions, 32 pieces: k_presence_expand<false>
        "ac500": stutter_query(rng, 500),             # 470 positions over a two-letter alphabet: many listed pieces
        "ac330": stutter_query(rng, 330),             # the same within 360 positions
        "read61": rand_seq(rng, 61),                  # 31 positions
        "rep1008": repeat_query(rng, 300, 438),       # 1008 positions: 63 pieces, rounded up to 64
        "rep1024": repeat_query(rng, 300, 454),       # 1024 positions: exactly 64 pieces
        "rep64": repeat_query(rng, 33, 28),           # 64 positions: G = 4
        "rep56": repeat_query(rng, 33, 20),           # 56 positions, a tail of 8
        # period 8 over the first 46 characters: positions 8 .. 15 repeat 0 .. 7 (a listed piece), 16 .. 31 are the unique k-mers 8 .. 23
        "per32": (rand_seq(rng, 8) * 6)[:46] + rand_seq(rng, 16),     # 32 positions: G = 2, delta == sub == 1
        "per16": (rand_seq(rng, 8) * 5)[:39] + rand_seq(rng, 7),      # 16 positions: one listed piece
        "run17": rand_seq(rng, 47),                   # 17 positions
        "run16": rand_seq(rng, 46),                   # 16 positions: G = 1
        "run9": rand_seq(rng, 39),
        "run1": rand_seq(rng, 31),
        "nohits": rand_seq(rng, 2000),                # longer than all of the small ones; never given a hit there
        # period 20: 20 unique k-mers however long the query, so the presence bits have 2 chunks where a hit has 32 or 128 pieces
        # (the kernel clamps the chunk a lane loads for the shuffles); position 20 t + 4 x starts a run of 16 one time in five
        "per300": (rand_seq(rng, 20) * 17)[:330],
        "per1070": (rand_seq(rng, 20) * 55)[:1100],
    }


def pieces_for(n):
    """`pieces` of a presence_hits call whose longest hit-bearing sequence has n positions: the power of two >= ceil(n / 16)."""
    p = 1
    while p * 16 < max(int(n), 1):
        p *= 2
    return p


def piece_classes(pos_map, pieces=None):
    """One dict per 16-position piece of a query with the position map `pos_map`: what k_presence_pieces records for it and which
    branches of k_presence_expand its thread takes in a call with `pieces` pieces per hit (default: the query's own, i.e. the query
    is the longest hit-bearing one of its batch).

      listed   the piece is not 16 (at the tail: cnt) consecutive unique indices: k_presence_expand_listed writes it
      otherwise j0 (unique index of its first position), delta = piece - (j0 >> 4), r = j0 & 15, sub = piece & (G - 1) with
      G = min(pieces, 64), cnt, and
      lo       "shuffle" (delta <= sub: the chunk is held by a lane of the same group) or "global"
      hi       "unused" (r == 0), "shuffle", or "global" (delta > sub + 1, or delta == 0 at the group's last lane)
      edge     delta == sub + 1 with r != 0: lo by global load, hi from the group's first lane
    """
    pm = np.asarray(pos_map, dtype=np.int64)
    n = pm.size
    pieces = pieces_for(n) if pieces is None else int(pieces)
    assert pieces & (pieces - 1) == 0 and pieces * 16 >= n
    G = min(pieces, 64)
    out = []
    for piece in range((n + 15) // 16):
        i0 = piece * 16
        cnt = min(16, n - i0)
        j0 = int(pm[i0])
        run = bool(np.array_equal(pm[i0:i0 + cnt], j0 + np.arange(cnt)))
        if not run:
            out.append({"piece": piece, "listed": True, "cnt": cnt})
            continue
        delta, r, sub = piece - (j0 >> 4), j0 & 15, piece & (G - 1)
        assert delta >= 0
        lo = "global" if delta > sub else "shuffle"
        hi = "unused" if r == 0 else "global" if (delta > sub + 1 or (delta == 0 and sub + 1 >= G)) else "shuffle"
        out.append({"piece": piece, "listed": False, "cnt": cnt, "j0": j0, "delta": delta, "r": r, "sub": sub, "G": G, "lo": lo, "hi": hi,
                    "edge": r != 0 and delta == sub + 1})
    return out


def class_names(pos_map, pieces=None):
    """The branch classes of piece_classes as a multiset {name: number of pieces}; the tests assert on these that their inputs
    reach every branch (never to compute expected output):
      listed | lo_shuffle | lo_global | hi_unused | hi_shuffle | hi_global | delta_eq_sub_plus_1 | delta_eq_sub_pos (delta == sub > 0:
      the farthest lane a shuffle may reach) | r0_lo_global (r == 0 with the chunk in another wavefront) | delta_pos (a run behind a
      repeat) | tail (cnt < 16) | tail_listed"""
    names = {}

    def add(name):
        names[name] = names.get(name, 0) + 1
    for p in piece_classes(pos_map, pieces):
        if p["cnt"] < 16:
            add("tail_listed" if p["listed"] else "tail")
        if p["listed"]:
            add("listed")
            continue
        add("lo_" + p["lo"])
        add("hi_" + p["hi"])
        if p["edge"]:
            add("delta_eq_sub_plus_1")
        if p["delta"] == p["sub"] > 0:
            add("delta_eq_sub_pos")
        if p["r"] == 0 and p["lo"] == "global":
            add("r0_lo_global")
        if p["delta"] > 0:
            add("delta_pos")
    return names
