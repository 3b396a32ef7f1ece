"""The cases of the top-N selection tests (a plain module: nothing here is collected): the numpy reference of k_rank_select, the tables
of cases that tests/test_rank_cases_host.py pins on the CPU and tests/test_gpu_rank_select.py runs on the device, and the staircase
indexes (tests/count_staircase.py, with chosen columns) of the end-to-end layer.

The rule (bigsi_kernels.hpp, K3r): the excluded colours are taken out of a query's hits; at most `limit` left: all of them stay;
otherwise an exact run keeps the `limit` lowest colours and a counting run the first `limit` of the order (count descending, colour
ascending).  Vectors are in row format: column 8b + j of a 64-bit word sits at bit 8b + 7 - j, i.e. the little-endian bytes of the
word are np.packbits of its 64 columns.

Layer D (DIRECT) feeds the kernel through bigsi_hip_rank_select_arrays: a case is ONE query -- hit columns, per-column counts (absent:
an exact run), num_unique, min_kmers -- plus what a call shares: wv, limit, the excluded colours and the counter width.  Cases with
the same shared part run as one call, one workgroup each.  A case declares the `edge` it is built for -- digit passes, the cutoff bin
of every pass, how many of the last bin still fit and how many it holds, the tile, thread and bit of the last tie kept and of the
first one dropped, the ties of earlier tiles (`base`) -- and analyse() recomputes those from the case's arrays by the kernel's own
steps; the host test compares the two.  Layer E (STAIR_CASES) runs limited searches on staircase indexes that carry a tie block."""
import numpy as np

import count_staircase as cs

DIGIT_BITS, BINS, TILE = 12, 4096, 256          # kRankDigitBits, kRankBins, kBlock: words per tile of the tie pass
JUNK16, JUNK32 = 0xFFFF, 0xFFFFFFFF             # what the counter of a column that is not a hit holds in layer D
PRESET = np.uint64(0xA5A5A5A55A5A5A5A)          # what an output buffer holds before the kernel runs


# --------------------------------------------------------------------------------------------- row format and the reference
def pack_cols(bits):
    """bool[64 * W] (by column) -> uint64[W] in row format"""
    bits = np.asarray(bits, bool)
    assert bits.size % 64 == 0
    return np.packbits(bits).view("<u8").astype(np.uint64)


def unpack_words(words):
    """uint64[W] in row format -> bool[64 * W] by column"""
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8)).astype(bool)


def words_of(cols, n_words):
    bits = np.zeros(64 * n_words, bool)
    cols = np.asarray(cols, np.int64)
    bits[cols[cols < bits.size]] = True          # (a colour beyond the vector has no bit: the host drops it, rank_select())
    return pack_cols(bits)


def ranked_order(cols, counts, excluded=(), exact=False):
    """The hit columns `cols` (any order) with their counts, excluded colours out, in the order a limited search cuts: exact --
    ascending colour; counting -- count descending, colour ascending."""
    cols = np.asarray(cols, np.int64)
    keep = ~np.isin(cols, np.asarray(list(excluded), np.int64))
    cols = cols[keep]
    if exact:
        return np.sort(cols)
    counts = np.asarray(counts, np.int64)[keep]
    return cols[np.lexsort((cols, -counts))]


def reference(hit_words, counts, nu, mk, excluded, limit, wv=None, preset=None):
    """What k_rank_select leaves for ONE query.  hit_words: uint64[stride] in row format, of which the first wv are the result (default:
    all); counts: int[64 * stride] by column, or None for an exact run; excluded: colours (those at or beyond 64 * wv are ignored).
    Returns uint64[stride]: the trimmed first wv words, the others as `preset` has them (default: as hit_words has them, the in-place
    run)."""
    hit_words = np.asarray(hit_words, np.uint64)
    wv = hit_words.size if wv is None else wv
    out = (hit_words if preset is None else np.asarray(preset, np.uint64)).copy()
    cols = np.flatnonzero(unpack_words(hit_words[:wv]))
    if counts is not None:
        c = np.asarray(counts, np.int64)[cols]
        assert ((c >= mk) & (c <= nu)).all(), "a hit's count lies in [min_kmers, num_unique]"
    order = ranked_order(cols, None if counts is None else c, excluded, counts is None)
    out[:wv] = words_of(order[:limit], wv)
    return out


# --------------------------------------------------------------------------------------------- the kernel's steps, for the edges
def analyse(c):
    """The branch quantities of a direct case, by the kernel's own steps (not through reference())."""
    wv, limit, mk = c["wv"], c["limit"], c["mk"]
    ex = {e for e in c["excluded"] if e < 64 * wv}
    cols = np.array(sorted(set(c["cols"].tolist()) - ex), np.int64)
    out = dict(total=int(cols.size), early=bool(cols.size <= limit), tiles=-(-wv // TILE))
    if out["early"]:
        return out
    remaining, bins, passes, hist_at = limit, [], 0, None
    ties = cols
    if c["counts"] is not None:
        v = np.maximum(c["counts"][cols] - mk, 0)
        rng = max(c["nu"] - mk, 0)
        bits = rng.bit_length() if rng else 1
        passes = -(-bits // DIGIT_BITS)
        prefix = mask = 0
        for shift in range((passes - 1) * DIGIT_BITS, -1, -DIGIT_BITS):
            cand = v[(v & mask) == prefix]
            hist = np.bincount((cand >> shift) & (BINS - 1), minlength=BINS)
            above = 0
            for b in range(BINS - 1, -1, -1):
                if above < remaining <= above + hist[b]:
                    break
                above += int(hist[b])
            bins.append(b)
            prefix |= b << shift
            mask |= (BINS - 1) << shift
            remaining -= above
            hist_at = int(hist[b])
        ties = cols[v == prefix]
        out.update(cutoff=prefix + mk, n_above=int((v > prefix).sum()))
    cut = int(ties[remaining - 1])
    drop = int(ties[remaining]) if remaining < ties.size else None
    where = lambda col: None if col is None else (col // 64 // TILE, col // 64 % TILE, col % 64)          # noqa: E731 -- (tile, thread, column of the word)
    out.update(limit=limit, passes=passes, bins=bins, remaining=int(remaining), hist=hist_at if hist_at is not None else int(ties.size), cut=where(cut),
               drop=where(drop), base=int((ties // 64 // TILE < cut // 64 // TILE).sum()), n_ties=int(ties.size))
    return out


# --------------------------------------------------------------------------------------------- layer D: the direct cases
def _d(group, name, wv, cols, counts, nu, mk, limit, excluded=(), cbytes=2, **edge):
    """One query.  cols: hit columns; counts: {column: count} or a count for all, None = exact."""
    cols = np.array(sorted(set(cols)), np.int64)
    assert cols.size == 0 or (0 <= cols[0] and cols[-1] < 64 * wv)
    full = None
    if counts is not None:
        full = np.full(64 * (wv + PAD), JUNK32 if cbytes == 4 else JUNK16, np.int64)
        full[cols] = [counts[int(x)] for x in cols] if isinstance(counts, dict) else counts
        assert nu <= (JUNK32 if cbytes == 4 else JUNK16)
    return dict(group=group, name=name, wv=wv, cols=cols, counts=full, nu=nu, mk=mk, limit=limit, excluded=tuple(excluded), cbytes=cbytes if counts is not None else 0,
                edge=edge)


PAD = 3          # words of a query behind wv: the stride of every direct call is wv + PAD, and nothing behind wv may change
RAGGED = 27      # the last word of a direct case holds 64 - RAGGED columns


def _ncols(wv):
    return 64 * wv - RAGGED


def call_key(c):
    """what a call of bigsi_hip_rank_select_arrays shares between its queries"""
    return (c["wv"], c["limit"], c["excluded"], c["cbytes"])


def _early():
    out = []
    for exact in (True, False):
        tag, cnt = ("x", None) if exact else ("c", {c: 40 + c % 3 for c in range(192)})
        kw = dict(counts=cnt, nu=50, mk=40, limit=5)
        hits7 = [3, 60, 63, 64, 100, 130, 164]
        out += [
            _d("early", "E%s_none" % tag, 3, [], early=True, total=0, **kw),
            _d("early", "E%s_below" % tag, 3, hits7[:4], early=True, total=4, **kw),
            _d("early", "E%s_at" % tag, 3, hits7[:5], early=True, total=5, **kw),
            _d("early", "E%s_above" % tag, 3, hits7[:6], early=False, total=6, **kw),
            # with excluded words: colours that are no hits (nothing changes), ...
            _d("early", "E%s_ex_idle_at" % tag, 3, hits7[:5], excluded=(5, 131), early=True, total=5, **kw),
            _d("early", "E%s_ex_idle_above" % tag, 3, hits7[:6], excluded=(5, 131), early=False, total=6, **kw),
            # ... and the exclusion alone bringing the total to the limit and below it: the copy must leave the excluded bits out
            _d("early", "E%s_ex_to_limit" % tag, 3, hits7[:6], excluded=(63,), early=True, total=5, **kw),
            _d("early", "E%s_ex_below" % tag, 3, hits7, excluded=(63, 64, 164), early=True, total=4, **kw),
            _d("early", "E%s_ex_still_above" % tag, 3, hits7, excluded=(64,), early=False, total=6, **kw),
            _d("early", "E%s_ex_all" % tag, 3, hits7[:3], excluded=(3, 60, 63), early=True, total=0, **kw),
        ]
    return out


def _exact_cut(name, wv, keep_last, drop_first, seed, only_from=0, **edge):
    """An exact run whose limit cuts between the hits keep_last and drop_first (no hit between them); other hits seeded, density 0.3,
    none below column `only_from`."""
    rng = np.random.default_rng(seed)
    n = _ncols(wv)
    bits = rng.random(n) < 0.3
    bits[:keep_last if only_from else 0] = False          # (only_from: keep_last is the first hit, the limit 1)
    assert not only_from or keep_last >= only_from
    bits[keep_last:drop_first + 1] = False
    bits[[keep_last, drop_first]] = True
    cols = np.flatnonzero(bits)
    where = lambda col: (col // 64 // TILE, col // 64 % TILE, col % 64)          # noqa: E731
    declared = edge.pop("limit", None)
    c = _d("exact", name, wv, cols.tolist(), None, 0, 0, int((cols <= keep_last).sum()), early=False, cut=where(keep_last), drop=where(drop_first), **edge)
    if declared is not None:
        c["edge"]["limit"] = declared
    return c


def _exact():
    out = [
        # one word: the first bit, the middle of a byte, the ragged word's last column
        _exact_cut("X1_first_bit", 1, 0, 1, 1),
        _exact_cut("X1_mid_byte", 1, 19, 20, 2),
        _exact_cut("X1_ragged", 1, 35, 36, 3),
        # two words: the last bit of word 0 | the first of word 1
        _exact_cut("X2_word_edge", 2, 63, 64, 4),
        _exact_cut("X2_first_bit_of_word", 2, 64, 65, 5),
        # 255 words: the lane 63 | 64 edge of the scan, the ragged last word
        _exact_cut("X255_lane_63_64", 255, 64 * 63 + 63, 64 * 64, 6),
        _exact_cut("X255_lane_63_64_gap", 255, 64 * 63 + 10, 64 * 64 + 50, 7),
        _exact_cut("X255_ragged", 255, 64 * 254 + 30, 64 * 254 + 36, 8),
        # 256 words: one full tile, the cut in its last word
        _exact_cut("X256_last_word", 256, 64 * 255 + 3, 64 * 255 + 4, 9, tiles=1),
        # 257 words: word 255 | 256 is the tile edge; the ragged word is tile 1; limit = 1 with the only hits in the last tile
        _exact_cut("X257_tile_edge", 257, 64 * 255 + 63, 64 * 256, 10, tiles=2),
        _exact_cut("X257_ragged", 257, 64 * 256 + 5, 64 * 256 + 6, 11, base_min=1),
        _exact_cut("X257_limit1_last_tile", 257, 64 * 256 + 2, 64 * 256 + 30, 12, only_from=64 * 256, base=0, limit=1),
        # 513 words: three tiles, the last one word wide
        _exact_cut("X513_tile_edge_0_1", 513, 64 * 255 + 60, 64 * 256 + 7, 13, tiles=3),
        _exact_cut("X513_tile_edge_1_2", 513, 64 * 511 + 63, 64 * 512, 14),
        _exact_cut("X513_limit1_last_tile", 513, 64 * 512 + 1, 64 * 512 + 2, 15, only_from=64 * 512, base=0, limit=1),
        _exact_cut("X513_mid_byte_tile1", 513, 64 * 300 + 42, 64 * 300 + 43, 16, base_min=1),
        # 600 words: lane 63 | 64 of the third tile, the ragged word, a cut in the first word
        _exact_cut("X600_lane_63_64_tile2", 600, 64 * 575 + 63, 64 * 576, 17, base_min=1),
        _exact_cut("X600_ragged", 600, 64 * 599 + 35, 64 * 599 + 36, 18),
        _exact_cut("X600_first_word", 600, 7, 8, 19),
        _exact_cut("X600_limit1_last_tile", 600, 64 * 512 + 9, 64 * 590, 20, only_from=64 * 512, base=0, limit=1),
    ]
    return out


def _digit_case(group, name, values, limit, rng_, mk=7, wv=3, cbytes=2, spread=5, **edge):
    """A counting case from `values` = [(v, how many)], v = count - min_kmers, of a query with num_unique - min_kmers == rng_: the
    columns go round-robin over the values (every value's columns interleave with the others') at every `spread`-th column."""
    order, left = [], [[v, n] for v, n in values]
    while any(n for _, n in left):
        for e in left:
            if e[1]:
                order.append(e[0])
                e[1] -= 1
    cols = [1 + spread * i for i in range(len(order))]
    assert cols[-1] < _ncols(wv)
    if limit >= len(cols):
        return None          # (the limit reaches the total: that is the early return, not a digit case)
    return _d(group, name, wv, cols, {c: mk + v for c, v in zip(cols, order)}, mk + rng_, mk, limit, cbytes=cbytes, early=False, **edge)


def _one_digit():
    g, R = "one digit", 4095
    out = [
        _digit_case(g, "D1_all_at_mk", [(0, 20)], 7, 100, passes=1, bins=[0], remaining=7, hist=20),
        _digit_case(g, "D1_all_at_num_unique", [(R, 20)], 7, R, passes=1, bins=[4095], remaining=7, hist=20),
        _digit_case(g, "D1_all_at_mk_range0", [(0, 9)], 4, 0, passes=1, bins=[0], remaining=4, hist=9),
        _digit_case(g, "D1_two_values", [(5, 10), (9, 10)], 13, 100, passes=1, bins=[5], remaining=3, hist=10),
        _digit_case(g, "D1_range4095_top", [(R, 3), (R - 1, 3), (0, 3)], 4, R, passes=1, bins=[4094], remaining=1, hist=3),
    ]
    for b in (0, 15, 16, 1023, 1024, 4095):
        # the cutoff in bin b, its neighbours on both sides occupied: thread b / 16 owns the bin (15 | 16: a thread's last and first
        # bin; 1023 | 1024: the last bin of wavefront 0's threads, the first of wavefront 1's)
        above = [(v, 2) for v in sorted({b + 1, R}) if b < v <= R]
        below = [(v, 2) for v in sorted({b - 1, 0}) if 0 <= v < b]
        n_above = 2 * len(above)
        for tag, rem in (("mid", 2), ("one", 1), ("all", 4)):
            out.append(_digit_case(g, "D1_bin%d_%s" % (b, tag), above + [(b, 4)] + below, n_above + rem, R, passes=1, bins=[b], remaining=rem, hist=4))
    return out


def _two_digits():
    g = "two digits"
    vals = [(8192, 2), (8191, 2), (4097, 2), (4096, 2), (4095, 2), (1, 2)]
    out = [
        # range 4096: the smallest range with two passes
        _digit_case(g, "D2_r4096_cut4096", [(4096, 2), (4095, 3), (0, 3)], 1, 4096, passes=2, bins=[1, 0], remaining=1, hist=2),
        _digit_case(g, "D2_r4096_all4096", [(4096, 2), (4095, 3), (0, 3)], 2, 4096, passes=2, bins=[1, 0], remaining=2, hist=2),
        _digit_case(g, "D2_r4096_cut4095", [(4096, 2), (4095, 3), (0, 3)], 4, 4096, passes=2, bins=[0, 4095], remaining=2, hist=3),
        _digit_case(g, "D2_r4096_cut0", [(4096, 2), (4095, 3), (0, 3)], 6, 4096, passes=2, bins=[0, 0], remaining=1, hist=3),
    ]
    # range 8192, the cutoff at each value in turn; 4096, 4097 and 8191 share the high digit and differ in the low one
    for i, (v, want) in enumerate(((8192, [2, 0]), (8191, [1, 4095]), (4097, [1, 1]), (4096, [1, 0]), (4095, [0, 4095]), (1, [0, 1]))):
        out.append(_digit_case(g, "D2_r8192_cut%d_one" % v, vals, 2 * i + 1, 8192, passes=2, bins=want, remaining=1, hist=2))
        out.append(_digit_case(g, "D2_r8192_cut%d_all" % v, vals, 2 * i + 2, 8192, passes=2, bins=want, remaining=2, hist=2))
    # 16-bit counters at their last value, 32-bit ones at the first values a uint16 cannot hold
    top16 = [(65535 - 10, 2), (65534 - 10, 2), (65279 - 10, 2), (4096, 2)]
    out += [
        _digit_case(g, "D2_u16_65535", top16, 1, 65525, mk=10, passes=2, bins=[65525 >> 12, 65525 & 4095], remaining=1, hist=2, cutoff=65535),
        _digit_case(g, "D2_u16_65534", top16, 3, 65525, mk=10, passes=2, bins=[65524 >> 12, 65524 & 4095], remaining=1, hist=2, cutoff=65534),
        _digit_case(g, "D2_u16_65279", top16, 6, 65525, mk=10, passes=2, bins=[65269 >> 12, 65269 & 4095], remaining=2, hist=2, cutoff=65279),
    ]
    top32 = [(65537 - 1, 2), (65536 - 1, 2), (65535 - 1, 2), (5, 2)]
    for i, cnt in enumerate((65537, 65536, 65535)):
        out.append(_digit_case(g, "D2_u32_%d" % cnt, top32, 2 * i + 1, 65536, mk=1, cbytes=4, passes=2, bins=[(cnt - 1) >> 12, (cnt - 1) & 4095], remaining=1, hist=2,
                               cutoff=cnt))
    return out


def _three_digits():
    g, T = "three digits", 1 << 24
    digits = lambda v: [v >> 24, (v >> 12) & 4095, v & 4095]          # noqa: E731
    out = []
    # range 2^24 - 1: 24 bits, still two passes
    vals = [(T - 1, 2), (T - 2, 2), (T - 1 - 4096, 2), (9, 2)]
    for i, (v, _) in enumerate(vals):
        out.append(_digit_case(g, "D3_r24m1_cut%d" % i, vals, 2 * i + 1, T - 1, mk=3, cbytes=4, passes=2, bins=digits(v)[1:], remaining=1, hist=2, cutoff=v + 3))
    # range 2^24: the first with three passes; 2^24 + 1: values on both sides of the third digit's first step
    for rng_, vals in ((T, [(T, 2), (T - 1, 2), (T - 2, 2), (4096, 2), (4095, 2)]), (T + 1, [(T + 1, 2), (T, 2), (T - 1, 2), (0, 2)])):
        for i, (v, _) in enumerate(vals):
            for tag, rem in (("one", 1), ("all", 2)):
                out.append(_digit_case(g, "D3_r%d_cut%d_%s" % (rng_ - T, v, tag), vals, 2 * i + rem, rng_, mk=3, cbytes=4, passes=3, bins=digits(v), remaining=rem, hist=2,
                                       cutoff=v + 3))
    # pairs that differ in the lowest digit only, in the middle one only, in the highest only
    a = 0x1234567
    vals = [(a + (1 << 24), 1), (a + (1 << 12), 1), (a + 1, 1), (a, 1), (a - 1, 1), (5, 1)]
    for i, (v, _) in enumerate(vals[:5]):
        out.append(_digit_case(g, "D3_pairs_cut%d" % i, vals, i + 1, 1 << 26, mk=3, cbytes=4, passes=3, bins=digits(v), remaining=1, hist=1, cutoff=v + 3))
    return out


def _ties():
    g = "tie geometry"
    out = []
    # ties (v = 5) interleaved with higher counts (v = 9) column by column, through a word edge and inside bytes
    cols = list(range(50, 80))
    cnt = {c: 7 + (9 if c % 2 else 5) for c in cols}
    for rem, cut, drop in ((1, 50, 52), (4, 56, 58), (7, 62, 64), (8, 64, 66), (14, 76, 78)):
        out.append(_d(g, "T_interleaved_%d" % rem, 3, cols, cnt, 107, 7, 15 + rem, early=False, passes=1, bins=[5], remaining=rem, hist=15,
                      cut=(0, cut // 64, cut % 64), drop=(0, drop // 64, drop % 64)))
    # 600 words: ties in tile 0 and tile 2 and none in tile 1, which holds higher and lower counts: `base` goes over an empty tile
    t0 = [64 * 10 + 5, 64 * 10 + 6, 64 * 250 + 63, 64 * 255 + 63]
    t2 = [64 * 512, 64 * 520 + 3, 64 * 520 + 4, 64 * 575 + 63, 64 * 576, 64 * 599 + 36]
    hi = [64 * 300 + i for i in (0, 7, 8, 63)] + [3, 64 * 580]
    lo = [64 * 400 + i for i in (0, 1)] + [64 * 11]
    cnt = {c: 7 + 5 for c in t0 + t2}
    cnt.update({c: 7 + 9 for c in hi})
    cnt.update({c: 7 + 1 for c in lo})
    every = t0 + t2 + hi + lo
    for rem, cut, drop in ((2, t0[1], t0[2]), (4, t0[3], t2[0]), (5, t2[0], t2[1]), (6, t2[1], t2[2]), (8, t2[3], t2[4]), (9, t2[4], t2[5])):
        out.append(_d(g, "T_tiles_0_2_rem%d" % rem, 600, every, cnt, 107, 7, len(hi) + rem, early=False, passes=1, bins=[5], remaining=rem, hist=10,
                      cut=(cut // 64 // TILE, cut // 64 % TILE, cut % 64), drop=(drop // 64 // TILE, drop // 64 % TILE, drop % 64),
                      base=4 if cut >= 64 * 512 else 0))
    # 32-bit counters, 513 words: ties in every tile, the cut on each tile edge and in the one-word last tile
    t = [64 * 255 + 63, 64 * 256, 64 * 511 + 63, 64 * 512, 64 * 512 + 36]
    cnt = {c: 70000 for c in t}
    cnt.update({c: 70001 for c in (64 * 100, 64 * 512 + 1)})
    for rem in (1, 2, 3, 4):
        cut, drop = t[rem - 1], t[rem]
        out.append(_d(g, "T_u32_tile_edges_rem%d" % rem, 513, list(cnt), cnt, 70010, 3, 2 + rem, cbytes=4, early=False, passes=2, remaining=rem, hist=5,
                      cut=(cut // 64 // TILE, cut // 64 % TILE, cut % 64), drop=(drop // 64 // TILE, drop // 64 % TILE, drop % 64),
                      base=sum(x // 64 // TILE < cut // 64 // TILE for x in t)))
    return out


def _excluded():
    g = "excluded colours"
    last = _ncols(3) - 1          # 164
    out = []
    # hits with the highest count at column 0, 63, 64 and the last column, all four excluded; a tie block below them
    hi, tie, lo = [0, 63, 64, last, 20, 100], [30, 31, 32, 70, 71, 140], [40, 41, 150]
    cnt = {c: 7 + 9 for c in hi}
    cnt.update({c: 7 + 5 for c in tie})
    cnt.update({c: 7 + 1 for c in lo})
    every = hi + tie + lo
    out += [
        _d(g, "XC_edges", 3, every, cnt, 107, 7, 4, excluded=(0, 63, 64, last), early=False, total=11, passes=1, bins=[5], remaining=2, hist=6, n_above=2),
        _d(g, "XC_edges_exact", 3, every, None, 0, 0, 4, excluded=(0, 63, 64, last), early=False, total=11, cut=(0, 0, 32), drop=(0, 0, 40)),
        # every hit of word 1 (64, 70, 71, 100): the word comes out empty, its ties do not count
        _d(g, "XC_whole_word", 3, every, cnt, 107, 7, 7, excluded=(64, 70, 71, 100), early=False, total=11, passes=1, bins=[5], remaining=3, hist=4, n_above=4,
           cut=(0, 0, 32), drop=(0, 2, 140 - 128)),
        _d(g, "XC_whole_word_exact", 3, every, None, 0, 0, 8, excluded=(64, 70, 71, 100), early=False, total=11, cut=(0, 0, 63), drop=(0, 2, 140 - 128)),
        # among the higher counts and inside the tie block: both move the cut
        _d(g, "XC_high_and_tie", 3, every, cnt, 107, 7, 7, excluded=(20, 31), early=False, total=13, passes=1, bins=[5], remaining=2, hist=5, n_above=5,
           cut=(0, 0, 32), drop=(0, 1, 70 - 64)),
        _d(g, "XC_tie_head", 3, every, cnt, 107, 7, 7, excluded=(30,), early=False, total=14, passes=1, bins=[5], remaining=1, hist=5, cut=(0, 0, 31), drop=(0, 0, 32)),
        # colours at and beyond 64 * wv have no bit in the excluded words: ignored
        _d(g, "XC_beyond", 3, every, cnt, 107, 7, 7, excluded=(192, 195, 64 * 3 + 64 * PAD, 10 ** 6, 30), early=False, total=14, passes=1, bins=[5], remaining=1, hist=5),
        # the ragged word's last column inside the tie block, on 257 words (tile 1)
        _d(g, "XC_ragged_tie", 257, [5, 64 * 256 + 30, 64 * 256 + 35, 64 * 256 + 36], {5: 16, 64 * 256 + 30: 12, 64 * 256 + 35: 12, 64 * 256 + 36: 12}, 107, 7, 2,
           excluded=(64 * 256 + 30,), early=False, total=3, passes=1, bins=[5], remaining=1, hist=2, cut=(1, 0, 35), drop=(1, 0, 36), base=0),
    ]
    return out


DIRECT = [c for c in _early() + _exact() + _one_digit() + _two_digits() + _three_digits() + _ties() + _excluded() if c is not None]
DIRECT_GROUPS = ("early", "exact", "one digit", "two digits", "three digits", "tie geometry", "excluded colours")
assert len({c["name"] for c in DIRECT}) == len(DIRECT) and {c["group"] for c in DIRECT} == set(DIRECT_GROUPS)


def fuzz_call(seed, n_seqs=512, wv=600, cbytes=2):
    """One seeded call of n_seqs queries (cbytes 0: exact): per query a populated width of 1 .. wv words, a hit density, and counts
    drawn from a handful of values (heavy ties) or from the whole range.  Returns dict(hits uint64[n, stride], counts or None, nu, mk,
    excluded colours, limit, wv, stride)."""
    rng = np.random.default_rng(seed)
    stride = wv + PAD
    limit = int(rng.choice([1, 2, 7, 64, 65, 300, 5000]))
    top = (JUNK32 if cbytes == 4 else JUNK16) - 1
    hits = np.zeros((n_seqs, 64 * stride), bool)
    counts = None if not cbytes else np.full((n_seqs, 64 * stride), top + 1, np.uint32 if cbytes == 4 else np.uint16)
    nu, mk = np.zeros(n_seqs, np.int64), np.zeros(n_seqs, np.int64)
    for q in range(n_seqs):
        width = int(rng.integers(1, wv + 1)) if q % 4 else wv
        n = 64 * width - int(rng.integers(0, 64))
        dens = float(rng.choice([0.002, 0.02, 0.3, 0.9, 1.0]))
        hits[q, :n] = rng.random(n) < dens
        if cbytes:
            mk[q] = int(rng.integers(0, 50))
            rng_ = int(rng.choice([0, 1, 3, 4095, 4096, 5000, 65000, min(top - 50, (1 << 24) + 5)]))
            nu[q] = mk[q] + rng_
            kind = int(rng.integers(0, 3))
            if kind == 0 or rng_ < 4:          # heavy ties: at most four values
                vals = rng.integers(0, rng_ + 1, size=4)
                v = vals[rng.integers(0, 4, size=64 * stride)]
            elif kind == 1:                    # a narrow band below the top: shared high digits
                v = rng_ - rng.integers(0, min(rng_, 40) + 1, size=64 * stride)
            else:
                v = rng.integers(0, rng_ + 1, size=64 * stride)
            counts[q][hits[q]] = (mk[q] + v)[hits[q]]
    hits[:, 64 * wv:] = rng.random((n_seqs, 64 * PAD)) < 0.5          # junk behind wv
    excluded = sorted(set(rng.integers(0, 64 * wv, size=int(rng.choice([0, 3, 400]))).tolist()))
    return dict(hits=np.stack([pack_cols(h) for h in hits]), counts=counts, nu=nu, mk=mk, excluded=tuple(excluded), limit=limit, wv=wv, stride=stride, cbytes=cbytes)


# --------------------------------------------------------------------------------------------- layer E: staircase indexes with a tie block
class RankStaircase(cs.Staircase):
    """A staircase whose columns are given: [(column, target, family)] (Staircase places them by the same bisection)."""

    def __init__(self, s, h, m, n_cols, thresholds, seed, columns):
        cs.Staircase.__init__(self, s, h, m, n_cols, thresholds, seed, columns=columns)


def tie_block(n_cols):
    """the columns of the tie block: 61 .. 66 (a word edge), 16 380 .. 16 390 where the index is that wide (words 255 | 256: the tile
    edge of a 32 832-column index and the last words of a 16 416-column shard), and the last columns of the ragged last word"""
    block = list(range(61, 67))
    if n_cols > 16390:
        block += list(range(16380, 16391))
    return block + list(range(n_cols - 4, n_cols))


def rank_columns(n_cols, u, mk, tie, highs, lows):
    """[(column, target, family)]: the tie block at (tie, early); columns of higher counts before, inside the gaps of and behind it;
    columns of lower counts that still hit; columns at mk - 1, which do not."""
    block = tie_block(n_cols)
    spots_hi = [0, 7, 8, 60, 67, 100, 127, 128, 191]
    spots_lo = [30, 31, 59, 68, 150, 151]
    spots_out = [40, 41, 160]
    if n_cols > 16390:
        spots_hi += [16300, 16379, 16391, 16415, 16416, 16500, 32767, 32768, 32800, n_cols - 5]
        spots_lo += [16383 - 64, 16392, 20000, 32769]
    else:
        spots_hi += [n_cols - 5, n_cols - 6]
    assert not set(block) & set(spots_hi + spots_lo + spots_out) and max(spots_hi + spots_lo + spots_out) < n_cols
    cols = [(c, tie, "early") for c in block]
    cols += [(c, highs[i % len(highs)], cs.FAMILIES[i % 3]) for i, c in enumerate(spots_hi)]
    cols += [(c, lows[i % len(lows)], cs.FAMILIES[(i + 1) % 3]) for i, c in enumerate(spots_lo)]
    cols += [(c, mk - 1, cs.FAMILIES[i % 3]) for i, c in enumerate(spots_out) if mk >= 1]
    return sorted(cols)


def _stair(name, base, route, mk_of, tie_of, highs_of, lows_of, exact=False, sparse=False, devices=None, main_pos=None, threshold0=False, fill_first=False):
    b = dict(cs.CASE_BY_NAME[base])
    if main_pos:
        b["main_pos"] = main_pos
        b["m"] = cs.LARGE_M
    b.update(name=name, base=base, route=route, mk_of=mk_of, tie_of=tie_of, highs_of=highs_of, lows_of=lows_of, exact=exact, sparse=sparse, devices=devices,
             threshold0=threshold0, fill_first=fill_first)
    return b


_small = dict(mk_of=lambda u: u // 4, tie_of=lambda u, mk: mk + 1, highs_of=lambda u, mk: [u, u - 1, mk + 2], lows_of=lambda u, mk: [mk])
# (the wide index: every other high column at u -- the hits of its exact run, among them 16 415 | 16 416, the last column of shard 0 and the first of shard 1)
_wide = dict(_small, highs_of=lambda u, mk: [u, u, u - 1, mk + 2])
_r = cs._route
STAIR_CASES = [
    _stair("E_sliced16", "S10b", _r(10, 96, 4), **_small),
    _stair("E_one_slice", "Uplain10", _r(10, 1), **_small),
    _stair("E_sparse", "Usparse16", _r(16, 1, block=64, deep=1), sparse=True, fill_first=True, mk_of=lambda u: 64, tie_of=lambda u, mk: mk + 1,
           highs_of=lambda u, mk: [u, u - 1, mk + 2], lows_of=lambda u, mk: [mk]),
    # u = 65 530 at threshold 0.0: min_kmers 0, every column a hit, the untouched ones one tie block at v = 0 -- two digits of 16-bit counters
    _stair("E_two_digits", "S16b", _r(16, 96, 10), main_pos=65533, threshold0=True, mk_of=lambda u: 0, tie_of=lambda u, mk: 4096,
           highs_of=lambda u, mk: [u, u - 1, 8192, 8191, 4097], lows_of=lambda u, mk: [4095, 1]),
    _stair("E_32bit", "S32", _r(32, 96, 10), mk_of=lambda u: 100, tie_of=lambda u, mk: 65536,
           highs_of=lambda u, mk: [u, u - 1, 65537], lows_of=lambda u, mk: [65535, mk + 4096, mk + 4095, mk]),
    _stair("E_wide", "Wide256", _r(12, 1, block=256, tiles=2), **_wide),
    _stair("E_wide_exact", "Wide256", None, exact=True, **_wide),
    _stair("E_group", "Wide256", None, devices=[0, 0], **_wide),
]
STAIR_BY_NAME = {c["name"]: c for c in STAIR_CASES}
_stairs = {}


def build_stair(name):
    """(case, staircase, queries, threshold): built once per process and shared.  E_wide, E_wide_exact and E_group share one."""
    c = STAIR_BY_NAME[name]
    key = (c["base"], c["main_pos"])
    if key not in _stairs:
        main = cs.make_main(c["main_pos"], c["seed"])
        u = cs.unique_count(main)
        mk = c["mk_of"](u)
        thr = 0.0 if c["threshold0"] else cs.threshold_for(u, mk)
        tie = c["tie_of"](u, mk)
        sc = RankStaircase(main, c["h"], c["m"], c["n_cols"], [thr], c["seed"], rank_columns(c["n_cols"], u, mk, tie, c["highs_of"](u, mk), c["lows_of"](u, mk)))
        _stairs[key] = (sc, [main] + cs.make_fillers(main, c["n_queries"] - 1, c["fmax"], c["seed"]), thr, tie)
    return (c,) + _stairs[key]


def stair_limits(sc, tie, counts, mk, exact=False, excluded=()):
    """The limits of a staircase case, from the main query's reference counts: the cut after every column of the tie block that ends a
    stretch of it or a word (61 | 62 mid byte, 63 | 64, 66 | ..., 16 383 | 16 384, the ragged word's columns), and T - 1, T, T + 1 of the
    main query's hit total.  An exact run's hits are the few columns at u: every limit from 1 to T + 1."""
    hit = np.flatnonzero(counts >= (sc.u if exact else mk))
    hit = hit[~np.isin(hit, list(excluded))]
    T = hit.size
    if exact:
        return list(range(1, T + 2))
    block = [c for c in tie_block(sc.n_cols) if c not in excluded]
    above, ties = int((counts[hit] > tie).sum()), hit[counts[hit] == tie]
    marks = [c for c in block if c in (61, 62, 63, 64, 66, 16380, 16383, 16384, 16390, sc.n_cols - 4, sc.n_cols - 2)]
    lims = {above + int((ties <= c).sum()) for c in marks} | {1, T - 1, T, T + 1}
    return sorted(x for x in lims if x >= 1)
