"""The query front end (K1) at its canonical-form and dedupe edges (a plain module: nothing here is collected): a plain-Python
reference of what K1 computes, and the table of cases (CASES) that tests/test_k1_cases_host.py pins on the CPU and
tests/test_gpu_k1_edges.py runs on the device.  No GPU, no oracle import: the host test holds this reference against the oracle, the
recorded reference-project data (tests/golden/g1_hash.json) and the CPU twin, so that three implementations meet in one place.

Why.  K1 holds three implementations of "the smaller of a k-mer and its reverse complement": byte-wise (use_revcomp: run-time k and
the build kernels), select-only on registers (RegKmer<31>::canonical_words: the wave and the global route) and the eight-word
big-endian compare on packed words (kmer31_canonical_premix: k_kmerize_lds<31> and k_reads_fused, every k = 31 production query).
s and its reverse complement r satisfy r[i] = comp(s[k-1-i]); comp is an involution, so s[i] != r[i] iff s[k-1-i] != r[k-1-i]:
differences come in mirrored pairs and the FIRST one lies at byte j <= ceil(k/2) - 1 (15 for k = 31, word 3).  On random ACGT j = 0
decides with probability 3/4 and j >= 8 (words 2, 3) with 4^-8: random input never reaches the late words, nor the four byte
alignments p & 3 the words are cut at, nor the tie.  The shapes below place every j, both outcomes and the tie at every alignment.

The dedupe keeps first occurrences by STRING equality; fingerprints (kmer31_fingerprint, folded FNV-1a) only pre-select.  The
collision pairs below are different k-mers with equal 32-bit fingerprints (a fixed-seed birthday search over 400 000 random k-mers;
kept as literals, the host test recomputes the fingerprints): a fingerprint-only dedupe merges them.

Reference (integers only), restating the reference project: complement A<->T, C<->G, every other byte itself; canonical(s) =
min(s, revcomp(s)), forward on a tie; MurmurHash3_x86_32 of the canonical bytes, seeds 0..h-1, read as signed 32 bits, Python's
floor-mod m; unique k-mers as QUERY strings in first-occurrence order; rep[p] the first position with position p's k-mer,
pos_unique[p] its unique index; min_kmers = ceil(u * threshold) in double."""
import math
import random

K = 31
M, H, N_COLS = 20011, 3, 128
K1_ELEMENTS, K1_WAVE, K1_LDS, K1_GLOBAL = 0, 1, 2, 3
NONE, BY_K1, SORT256, SORT1024 = 0, 1, 2, 3
READS_MAX_POS, LDS_MAX_POS = 63, 4096
ARG_READ, ARG_SMALL, ARG_LARGE = 96, 1024, 3072
THRESHOLDS = (1.0, 0.5, 0.0)

# --------------------------------------------------------------------------------------------- the reference
def ceil_thr(u, thr):
    """min_kmers = ceil(u * threshold) in IEEE double, as Python evaluates int * float; a negative bound behaves like 0
    (count_staircase.min_kmers, restated so that this module imports nothing of the project: the host test holds the two together)"""
    return max(int(math.ceil(u * thr)), 0)


HOMOPOLYMER_SIZES = (1, 63, 64, 65, 256, 1024, 1025, 4096, 4097)
_COMP = {"A": "T", "T": "A", "C": "G", "G": "C"}


def complement(c):
    return _COMP.get(c, c)


def revcomp(s):
    return "".join(complement(c) for c in reversed(s))


def canonical(s):
    r = revcomp(s)
    return r if r < s else s          # (ASCII strings compare as their bytes do)


def murmur3_32(data, seed):
    """MurmurHash3_x86_32 of a bytes object: the unsigned 32-bit value"""
    c1, c2, mask = 0xcc9e2d51, 0x1b873593, 0xFFFFFFFF
    h1, n = seed & mask, len(data)
    for i in range(0, n - n % 4, 4):
        k1 = int.from_bytes(data[i:i + 4], "little")
        k1 = (k1 * c1) & mask
        k1 = ((k1 << 15) | (k1 >> 17)) & mask
        k1 = (k1 * c2) & mask
        h1 ^= k1
        h1 = ((h1 << 13) | (h1 >> 19)) & mask
        h1 = (h1 * 5 + 0xe6546b64) & mask
    if n % 4:
        k1 = int.from_bytes(data[n - n % 4:], "little")
        k1 = (k1 * c1) & mask
        k1 = ((k1 << 15) | (k1 >> 17)) & mask
        k1 = (k1 * c2) & mask
        h1 ^= k1
    h1 ^= n
    h1 ^= h1 >> 16
    h1 = (h1 * 0x85ebca6b) & mask
    h1 ^= h1 >> 13
    h1 = (h1 * 0xc2b2ae35) & mask
    h1 ^= h1 >> 16
    return h1


def signed_hash(s, seed):
    """mmh3.hash(s, seed): signed 32 bits"""
    v = murmur3_32(s.encode("ascii"), seed)
    return v - (1 << 32) if v >= 1 << 31 else v


def kmer_rows(kmer, h, m):
    c = canonical(kmer)
    return [signed_hash(c, seed) % m for seed in range(h)]


class Ref(object):
    """K1's outputs for one sequence: n, u, uniq (the unique k-mers), first (their first positions), rep, pos_unique, and
    rows(h, m) -> [u][h]"""

    def __init__(self, seq, k):
        self.seq, self.k = seq, k
        self.n = n = max(len(seq) - k + 1, 0)
        seen, self.uniq, self.first, self.rep, self.pos_unique = {}, [], [], [], []
        for p in range(n):
            km = seq[p:p + k]
            if km not in seen:
                seen[km] = len(self.uniq)
                self.uniq.append(km)
                self.first.append(p)
            self.pos_unique.append(seen[km])
            self.rep.append(self.first[seen[km]])
        self.u = len(self.uniq)
        self._rows = {}

    def rows(self, h, m):
        if (h, m) not in self._rows:
            self._rows[(h, m)] = [kmer_rows(km, h, m) for km in self.uniq]
        return self._rows[(h, m)]


_refs = {}


def ref_of(seq, k):
    """computed once per (sequence, k), shared, never changed"""
    if (seq, k) not in _refs:
        _refs[(seq, k)] = Ref(seq, k)
    return _refs[(seq, k)]


def first_difference(kmer):
    """(j, who): the first byte at which the k-mer differs from its reverse complement and who is smaller there ("fwd" / "rc");
    (None, "tie") for a k-mer that is its own reverse complement"""
    r = revcomp(kmer)
    for j, (a, b) in enumerate(zip(kmer, r)):
        if a != b:
            return j, ("fwd" if a < b else "rc")
    return None, "tie"


# --------------------------------------------------------------------------------------------- the dedupe fingerprints, restated
def fnv_fold(kmer):
    """fnv1a of bigsi_kernels.hpp: FNV-1a over the bytes, folded by h ^ (h >> 15)"""
    h = 2166136261
    for c in kmer.encode("ascii"):
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h ^ (h >> 15)


def fp31(kmer):
    """kmer31_fingerprint: eight little-endian words (the last holds 3 bytes), multiply-xor, folded"""
    assert len(kmer) == 31
    b, fp = kmer.encode("ascii") + b"\0", 0
    for i in range(8):
        fp = ((fp ^ int.from_bytes(b[4 * i:4 * i + 4], "little")) * 0x9E3779B1) & 0xFFFFFFFF
    return fp ^ (fp >> 15)


# pairs of DIFFERENT k-mers with equal fingerprint, and k-mers whose fingerprint ends in ten one bits (their home slot is the last
# of any dedupe table of at most 1024 slots)
FP31_PAIRS = [("AAACTAAAGAACTTCGAGGGAGCTGATTTCC", "TAAAAAAAAGTTGCCATTTAAGGAGAGGTAC"), ("AGTACGTAAACTGACAGGACTACCACCCTTT", "CTGATCAGAGGTTTTGCAATGGGCGTAACAT"),
              ("TTCTGCTACTGTAGACGACCAGAGGGACTCG", "CACGGGTTAGCAACAGCTCTCAGATGGTTGG")]
FNV31_PAIRS = [("AGTTAGCTCTACGGTGAGTTTCGTGCCGGTA", "CGCAAGCGTCGAGTCTCTGGCTGTCTAAATG"), ("CCAGGGTACTGCTCTCTCCGGTTAATTTGAG", "TGGATGTACAGTCCAAGATCAGTCCATATCA"),
               ("ATCCCAACGGTACTTTTGAAGAACGCGATTC", "AATCGTAGTGTATCTTAAGTCCTGGGTTACT")]
FNV21_PAIRS = [("TGCCGGCCCAAGCACTGTTGA", "AACAACAGCCAACCCAGCGCG"), ("CATGATACTCCGGAGGAACCG", "AGCCACGCAAACCGTTCTATT"),
               ("CCTGCCTAGAGGAACTAGTTA", "CTCTCGTGGTTAAATGTATTG")]
FP31_LAST = ["TCAAACGCTTAGGTGATCGCAATGGGATGCT", "CCTTATCTTACGTTCGTATAGTCGTCTGGCC", "TGGCTTACACGAGTCCCCCTTACTAGGTATC", "TCGTGCCTCCTGATTGCGAGTGATGGTTTCA"]
FNV31_LAST = ["GCGTGTTTACGGAAGGAGCGTCAACGCTCCC", "ACCTGATTATATGTATAACGACGGTATCCGT", "AATTTAGCTTTACAGGATATACTTGACCCTA", "CATCGCGACTATTTTCTACAAAGGGTTCTAA"]
FNV21_LAST = ["CTTGCTGATATAGGCTTTCGC", "TTTTTGTCACATGATGAGGCA", "TCTAAGACAATAACTGTATCG", "TGTCCATTTTGAACACTCAGG", "GTTCCGGTTCAACCCTTATAA"]


def k1_table_slots(positions, tab_mult):
    t = 2
    while t < tab_mult * positions:
        t <<= 1
    return t


def global_table_slots(positions):
    t = 1
    while t < 2 * positions:
        t <<= 1
    return t


def replay_inserts(seq, k, slots, fingerprint):
    """the dedupe table after inserting the positions of seq in order (open addressing, linear probing, a slot keeps the first
    position of its k-mer): list of positions, None for an empty slot"""
    tab, mask = [None] * slots, slots - 1
    for p in range(max(len(seq) - k + 1, 0)):
        km = seq[p:p + k]
        s = fingerprint(km) & mask
        while tab[s] is not None and seq[tab[s]:tab[s] + k] != km:
            s = (s + 1) & mask
        if tab[s] is None:
            tab[s] = p
    return tab


# --------------------------------------------------------------------------------------------- the launch rule's K1 part, restated
def k1_plan(n_seqs, max_pos, max_len, force_global):
    """k1_plan of bigsi_launch.hpp: (route, tab_mult)"""
    if not force_global and max_pos <= 64:
        return K1_WAVE, 4
    hs_cap = -(-max(max_pos, 1) // 4) * 4
    sq_bytes = -(-(max_len + 16) // 16) * 16
    tab_mult = 8 if n_seqs <= 32 else 4
    while True:
        cap = 2
        while cap < tab_mult * max_pos and cap < 1 << 30:
            cap <<= 1
        lds = (cap + cap // 32 + 4) * 4 + 64 + hs_cap * 4 + 2 * sq_bytes
        if lds <= 60 * 1024 or tab_mult == 2:
            break
        tab_mult //= 2
    return (K1_LDS if not force_global and max_pos <= LDS_MAX_POS and lds <= 60 * 1024 else K1_GLOBAL), tab_mult


def expected_route(queries, k, h, n_cols, thr, run_kw, one_call=False):
    """What a run must report (bigsi_hip_batch_last_row_and, bigsi_hip_hits_last_path): the conditions of reads_fusable, k1_plan,
    plan_row_and's want_sorted and run_kmerize's workgroup size, parts and argument class, restated.  The host test holds the K1
    route, the table multiplier and the sort's workgroup against the compiled planner."""
    n = len(queries)
    pos = [max(len(q) - k + 1, 0) for q in queries]
    max_pos, max_len, wv = max(pos), max(len(q) for q in queries), -(-n_cols // 64)
    exact, glob = thr == 1.0, bool(run_kw.get("k1_global"))
    one_len = max_len if one_call and n == 1 else 0
    if (k == 31 and sum(pos) > 0 and max_pos <= READS_MAX_POS and wv <= 512 and 2 <= h <= 4 and not glob and
            (exact or run_kw.get("sparse_counts"))):
        return dict(one_launch=1, k1_route=0, k1_parts=1, k1_arg_bytes=ARG_READ if 0 < one_len <= ARG_READ else 0, sorted_by=NONE, zero_copy=0,
                    instance="k_reads_fused", block=256, tab_mult=0)
    route, tab_mult = k1_plan(n, max_pos, max_len, glob)
    want_sorted = exact and n * -(-wv // 128) >= 1024 and max_pos * h >= 1024
    out = dict(one_launch=0, k1_route=route, k1_parts=1, k1_arg_bytes=0, zero_copy=int(one_call and route != K1_GLOBAL), block=256, tab_mult=tab_mult)
    kf = "31" if k == 31 else "0"
    if route == K1_LDS:
        cap, block = (256 if n >= 1024 else 1024), 64
        while block < max_pos and block < cap:
            block <<= 1
        out["block"] = block
        if not want_sorted and 256 <= max_pos <= block and n <= 32:
            out["k1_parts"] = 8
        out["k1_arg_bytes"] = 0 if not one_len else ARG_SMALL if one_len <= ARG_SMALL else ARG_LARGE if one_len <= ARG_LARGE else 0
        out["sorted_by"] = BY_K1 if want_sorted else NONE
        out["instance"] = "k_kmerize_lds<%s>" % kf
    else:
        out["sorted_by"] = NONE if not want_sorted else SORT1024 if max_pos * h >= 2048 else SORT256
        out["instance"] = ("k_kmerize_wave<%s>" if route == K1_WAVE else "k_kmer_rows<%s>") % kf
    return out


# --------------------------------------------------------------------------------------------- A: the canonical shapes
def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def make_shape(k, j, who, rng):
    """A k-mer whose first difference from its reverse complement is at byte j, decided for `who`; (None, "tie"): its own reverse
    complement.  left + centre + revcomp(left) over the alphabet CG is a palindrome (centre N for odd k: N complements to itself);
    byte j set to A makes the k-mer the smaller one there, T the reverse complement (the mirrored byte k-1-j differs too, later)."""
    left = _rand(rng, k // 2, "CG")
    s = list(left + ("N" if k % 2 else "") + revcomp(left))
    if who != "tie":
        s[j] = "A" if who == "fwd" else "T"
    s = "".join(s)
    assert len(s) == k and first_difference(s) == (j, who), (s, j, who)
    assert canonical(s) == (revcomp(s) if who == "rc" else s)
    return s


def make_shapes(k, js, seed):
    rng = random.Random(seed)
    return [((j, who), make_shape(k, j, who, rng)) for j in js for who in ("fwd", "rc")] + [((None, "tie"), make_shape(k, None, "tie", rng))]


SHAPES = make_shapes(K, range(16), 31)                  # 33 of them: [((j, who), k-mer)]
SHAPE_OF = dict(SHAPES)
assert len(SHAPE_OF) == 33 and len(set(SHAPE_OF.values())) == 33
PLACEMENTS = [(key, a) for key, _ in SHAPES for a in range(4)]          # (shape, alignment p & 3): 132


def deep(key):
    return key[0] is not None and key[0] >= 8


def place(rng, items, k=K, shapes=None, tail=0, extra=None):
    """One sequence holding the k-mers `items` = [(shape key, alignment)] in order: each starts at a byte offset p with p & 3 == its
    alignment, 1..4 random spacer bytes in between (0..3 before the first; extra[i] more before item i); `tail` random bytes behind
    the last.  Returns (sequence, [position of every item])."""
    shapes = shapes or SHAPE_OF
    s, at = "", []
    for i, (key, a) in enumerate(items):
        s += _rand(rng, extra[i] if extra else 0)
        pad = (a - len(s)) % 4
        if i and pad == 0:
            pad = 4
        s += _rand(rng, pad)
        at.append(len(s))
        s += shapes[key]
    return s + _rand(rng, tail), at


def read_queries(seed=7):
    """66 queries of at most 93 bytes holding the 132 placements, two each: the first at p = 0..3 (p = 0: the first position of its
    sequence), the second at the LAST position of its sequence"""
    rng, out = random.Random(seed), []
    for i in range(0, len(PLACEMENTS), 2):
        s, at = place(rng, PLACEMENTS[i:i + 2])
        assert len(s) <= 93 and at[1] == len(s) - K and at[0] == PLACEMENTS[i][1]
        out.append(s)
    return out


def packed_queries(rng, items, max_len, min_len=0, k=K, shapes=None):
    """`items` packed greedily into sequences of at most max_len bytes (at least min_len: random bytes appended)"""
    out, cur = [], []
    for it in items:
        s, _ = place(rng, cur + [it], k, shapes)
        if cur and len(s) > max_len:
            out.append(cur)
            cur = []
        cur.append(it)
    out.append(cur)
    seqs = []
    for group in out:
        s, _ = place(random.Random(rng.random()), group, k, shapes)
        seqs.append(s + _rand(rng, max(min_len - len(s), 0)))
        assert min_len <= len(seqs[-1]) <= max(max_len, min_len)
    return seqs


def placements_in(queries, k=K):
    """{(j, who, p & 3)} over every k-mer position of the queries, from the reference alone"""
    got = set()
    for q in queries:
        for p in range(max(len(q) - k + 1, 0)):
            j, who = first_difference(q[p:p + k])
            got.add((j, who, p & 3))
    return got


ALL_PLACEMENTS = {(j, who, a) for (j, who), a in PLACEMENTS}


# --------------------------------------------------------------------------------------------- B: dedupe
def repeat_query(rng, n, pairs, k):
    """n positions of random ACGT in which, for every (p1, p2) of `pairs`, the k-mer at p1 comes back at p2 (p2 - p1 >= k)"""
    while True:
        s = list(_rand(rng, n + k - 1))
        for p1, p2 in sorted(pairs):
            assert p2 - p1 >= k and p2 < n
            s[p2:p2 + k] = s[p1:p1 + k]
        s = "".join(s)
        r = Ref(s, k)
        if all(r.rep[p2] == p1 for p1, p2 in pairs):        # (else a chance third copy: draw again)
            return s


def homopolymer(n, k, c="A"):
    return c * (n + k - 1)


def strand_queries(rng, k):
    """period 2 and 3; X + revcomp(X): two uniques with equal rows; X, X in lower case, X with an N: three uniques"""
    x = _rand(rng, k)
    xn = x[:k // 2] + "N" + x[k // 2 + 1:]
    return ["AC" * 20 + "A" * (k % 2), ("ACG" * 24)[:k + 30], x + revcomp(x), x + x.lower() + xn]


def abab(pairs):
    return [a + b + a + b for a, b in pairs]


def aba(pairs):
    """(the wave route and the read kernel hold 64 / 63 positions: A + B + A + B does not fit; both orders instead)"""
    return [q for a, b in pairs for q in (a + b + a, b + a + b)]


def wrap_query(last, k, fingerprint, slot_counts):
    """the k-mers `last` (all at home in the last slot of every table of slot_counts) in the first order in which a sequential
    insert of the whole sequence leaves the last slot to its first k-mer and slot 0 to another of them: the chain wraps"""
    import itertools
    for perm in itertools.permutations(last):
        q = "".join(perm)
        tabs = [replay_inserts(q, k, s, fingerprint) for s in slot_counts]
        if all(t[-1] == 0 and t[0] is not None and q[t[0]:t[0] + k] in perm[1:] for t in tabs):
            return q
    raise AssertionError("no order of the k-mers wraps into slot 0")


def isolate(queries, k):
    """a sequence shorter than k and an empty one at the first, a middle and the last batch position; the first query twice"""
    mid = len(queries) // 2
    return ["A" * (k - 1), ""] + queries[:mid] + ["", "C" * max(k - 2, 0), queries[0]] + queries[mid:] + ["G" * (k - 1), ""]


# --------------------------------------------------------------------------------------------- the case table
def _case(name, built_for, queries, k=K, h=H, m=M, runs=None, kind="batch", note=""):
    runs = runs or [(thr, {}) for thr in THRESHOLDS]
    return dict(name=name, built_for=built_for, queries=queries, k=k, h=h, m=m, n_cols=N_COLS, runs=runs, kind=kind, note=note)


def _fillers(rng, n, length=K):
    return [_rand(rng, length) for _ in range(n)]


def _build_cases():
    rng = random.Random(2031)
    cases = []
    # ---- A, reads: 1024 queries; the 66 shape queries stand at 0.., 256.., 512.., 768..: the read kernel rotates its two K1
    # wavefronts with q >> 8.  Five ways through the same batch (the h = 1 index is a case of its own).
    rq = read_queries()
    short = strand_queries(rng, K) + aba(FP31_PAIRS) + aba(FNV31_PAIRS) + [homopolymer(1, K), homopolymer(63, K), repeat_query(rng, 63, [(0, 62)], K), repeat_query(rng, 63, [(0, 31)], K)]
    assert all(len(q) <= 93 for q in rq + short)
    reads = []
    for blk in range(4):
        body = rq + short
        reads += body + _fillers(rng, 256 - len(body))
    assert len(reads) == 1024 and all(reads[256 * b] == rq[0] for b in range(4))
    five = [(1.0, {}), (0.5, dict(sparse_counts=True)), (0.5, {}), (0.0, {}), (1.0, dict(k1_global=True))]
    cases.append(_case("reads", ["k_reads_fused", "k_reads_fused", "k_kmerize_wave<31>", "k_kmerize_wave<31>", "k_kmer_rows<31>"], reads, runs=five))
    cases.append(_case("reads_h1", ["k_kmerize_wave<31>"] * 3, reads, h=1))
    cases.append(_case("reads_isolated", ["k_reads_fused", "k_reads_fused", "k_kmerize_wave<31>"], isolate(rq[:6] + short[:4], K),
                       runs=[(1.0, {}), (0.5, dict(sparse_counts=True)), (0.0, {})]))
    # ---- the wave route's lane 63: queries of exactly 64 positions, a shape at the last one (alignment 3), a repeat into lane 63
    wave64 = []
    for i, key in enumerate([(15, "fwd"), (15, "rc"), (None, "tie"), (8, "rc"), (11, "fwd")]):
        s, at = place(rng, [(SHAPES[(5 * i) % 33][0], i % 4), (key, 3)])
        s = s[:at[1]] + _rand(rng, 63 - at[1]) + SHAPE_OF[key]
        assert len(s) == 94 and s[63:] == SHAPE_OF[key]
        wave64.append(s)
    wave64 += [homopolymer(64, K), repeat_query(rng, 64, [(0, 63)], K), repeat_query(rng, 64, [(32, 63)], K)] + aba(FNV31_PAIRS) + short[:4]
    cases.append(_case("wave64", ["k_kmerize_wave<31>"] * 3, isolate(wave64, K)))
    # ---- A, LDS: the placements packed into queries of 65 .. 200 positions
    lds = packed_queries(rng, PLACEMENTS, 200, 95)
    assert len(lds) <= 27 and all(65 <= len(q) - K + 1 <= 200 for q in lds)
    cases.append(_case("lds_shapes", ["k_kmerize_lds<31>"] * 3, isolate(lds, K)))
    # ---- B, LDS with one pass and one part (at most 32 queries of fewer than 256 positions: 8 slots per position)
    wrap31 = wrap_query(FP31_LAST, K, fp31, (1024, 512))          # (94 positions: 8 or 4 slots per position)
    dedupe = ([homopolymer(65, K), repeat_query(rng, 200, [(0, 199), (32, 63), (33, 64), (100, 140)], K), wrap31] + strand_queries(rng, K) +
              abab(FP31_PAIRS) + abab(FNV31_PAIRS))
    cases.append(_case("lds_dedupe", ["k_kmerize_lds<31>"] * 3, isolate(dedupe, K)))
    cases.append(_case("global_dedupe", ["k_kmer_rows<31>"] * 3, isolate(dedupe + [wrap_query(FNV31_LAST, K, fnv_fold, (256,))] + lds[:4] + [homopolymer(n, K) for n in HOMOPOLYMER_SIZES[:-1] if n != 65], K), runs=[(t, dict(k1_global=True)) for t in THRESHOLDS]))
    # ---- parts = 8: at most 32 queries, 256 <= max_pos <= 1024.  Four queries of eight segments, segment i holding both shapes of
    # j = 8 + i (unique k-mers number about 94 i .. 94 i + 93 of about 750: part i of 8); repeats either side of a share boundary
    # (n = 512: shares of 64 positions)
    parts = []
    for r in range(4):
        items = [((8 + i, who), (r + i + d) % 4) for i in range(8) for d, who in enumerate(("fwd", "rc"))]
        parts.append(place(rng, items, extra=[28 * (i % 2 == 0 and i > 0) for i in range(16)], tail=28)[0])
    parts += [homopolymer(256, K), homopolymer(1024, K), repeat_query(rng, 512, [(10, 64), (63, 100), (0, 511), (127, 448)], K)] + abab(FP31_PAIRS[:1]) + strand_queries(rng, K)
    cases.append(_case("lds_parts8", ["k_kmerize_lds<31>"] * 3, isolate(parts, K)))
    # ---- the second pass of a 1024-thread workgroup (more than 1024 positions: the pass probes instead of reading my_slot)
    cases.append(_case("lds_pass2", ["k_kmerize_lds<31>"] * 2,
                       [homopolymer(1025, K), repeat_query(rng, 1100, [(5, 1029), (0, 1099), (1023, 1060)], K), homopolymer(4096, K), lds[0]],
                       runs=[(1.0, {}), (0.5, {})]))
    many31 = [homopolymer(256, K), homopolymer(1024, K), repeat_query(rng, 1024, [(0, 1023), (511, 600)], K)] + strand_queries(rng, K) + abab(FP31_PAIRS[:1]) + _fillers(rng, 30, 50)
    cases.append(_case("lds_many", ["k_kmerize_lds<31>"] * 2, isolate(many31, K), runs=[(1.0, {}), (0.5, {})]))
    # ---- 1024 queries: workgroups of 256 threads, 4 slots per position; exact: the fused row sort (one query of 342 positions or
    # more makes the row lists long enough for the planner); a long query between short ones
    sort_q = lds + [repeat_query(rng, 300, [(5, 261), (0, 299)], K), homopolymer(256, K), homopolymer(1024, K), wrap31, _rand(rng, 400 + K - 1)] + abab(FP31_PAIRS) + strand_queries(rng, K)
    many = _fillers(rng, 3) + [""] + sort_q + _fillers(rng, 1024 - len(sort_q) - 6) + ["A" * 30, _rand(rng, 380)]
    assert len(many) == 1024
    cases.append(_case("lds_sorted", ["k_kmerize_lds<31>"] * 2, many, runs=[(1.0, {}), (0.5, {})]))
    # ---- the global route by length
    cases.append(_case("global_long", ["k_kmer_rows<31>"] * 2, [lds[1], homopolymer(4097, K), "", repeat_query(rng, 4100, [(0, 4099), (2000, 4000)], K), lds[2]],
                       runs=[(1.0, {}), (0.5, {})]))
    # ---- B at k = 21: the KF = 0 instances
    k = 21
    short21 = strand_queries(rng, k) + aba(FNV21_PAIRS) + [homopolymer(1, k), homopolymer(63, k), homopolymer(64, k), repeat_query(rng, 64, [(0, 63), (21, 42)], k)]
    cases.append(_case("wave_k21", ["k_kmerize_wave<0>"] * 3, isolate(short21, k), k=k))
    long21 = [homopolymer(65, k), repeat_query(rng, 200, [(0, 199), (32, 63), (33, 64), (100, 140)], k), wrap_query(FNV21_LAST, k, fnv_fold, (1024, 256))] + abab(FNV21_PAIRS) + strand_queries(rng, k)
    cases.append(_case("lds_k21", ["k_kmerize_lds<0>"] * 3, isolate(long21, k), k=k))
    cases.append(_case("global_k21", ["k_kmer_rows<0>"] * 3, isolate(long21 + short21[:3] + [homopolymer(n, k) for n in HOMOPOLYMER_SIZES[:-1] if n != 65], k), k=k, runs=[(t, dict(k1_global=True)) for t in THRESHOLDS]))
    cases.append(_case("lds_parts8_k21", ["k_kmerize_lds<0>"] * 2, isolate([homopolymer(256, k), repeat_query(rng, 512, [(10, 64), (63, 100), (0, 511)], k), homopolymer(1024, k)] + strand_queries(rng, k) + abab(FNV21_PAIRS[:1]), k),
                       k=k, runs=[(1.0, {}), (0.5, {})]))
    # ---- one part, one full pass of 1024 threads: more than 32 queries (4 slots per position), up to 1024 positions
    many21 = [homopolymer(256, k), homopolymer(1024, k), repeat_query(rng, 1024, [(0, 1023), (511, 600)], k)] + strand_queries(rng, k) + abab(FNV21_PAIRS[:1]) + _fillers(rng, 30, 40)
    cases.append(_case("lds_many_k21", ["k_kmerize_lds<0>"] * 2, isolate(many21, k), k=k, runs=[(1.0, {}), (0.5, {})]))
    cases.append(_case("lds_pass2_k21", ["k_kmerize_lds<0>"], [homopolymer(1025, k), repeat_query(rng, 1100, [(5, 1029), (0, 1099)], k), homopolymer(4096, k)], k=k, runs=[(0.5, {})]))
    cases.append(_case("global_long_k21", ["k_kmer_rows<0>"], [homopolymer(4097, k), long21[1]], k=k, runs=[(1.0, {})]))
    # ---- C: run-time k.  Per k the shapes of j = 0, one in between and ceil(k / 2) - 1, both outcomes, and the tie: one per query
    # on the wave route, all in one query on the LDS route, both again on the global route
    for k in RUNTIME_KS:
        shapes = RUNTIME_SHAPES[k]
        sd = dict(shapes)
        singles = [place(rng, [(key, i % 4)], k, sd, tail=i % 3)[0] for i, (key, _) in enumerate(shapes)]
        items = [(key, a) for a in range(4) for key, _ in shapes]
        long_q = packed_queries(rng, items, 4000, 66 + k, k, sd)
        assert len(long_q) == 1 and len(long_q[0]) - k + 1 >= 65
        cases.append(_case("k%d_wave" % k, ["k_kmerize_wave<0>"] * 3, isolate(singles, k), k=k))
        cases.append(_case("k%d_lds" % k, ["k_kmerize_lds<0>"] * 2, long_q + singles[:2], k=k, runs=[(1.0, {}), (0.5, {})]))
        cases.append(_case("k%d_global" % k, ["k_kmer_rows<0>"], long_q + singles, k=k, runs=[(1.0, dict(k1_global=True))]))
    # ---- D: the modulus.  m = 2 and 7 on every instance (the read kernel; wave, LDS with one and eight parts, global at both KF)
    for m in (2, 7):
        cases.append(_case("m%d_reads" % m, ["k_reads_fused", "k_kmerize_wave<31>", "k_kmer_rows<31>"], rq[:12] + short[:4], m=m,
                           runs=[(1.0, {}), (0.5, {}), (1.0, dict(k1_global=True))]))
        cases.append(_case("m%d_lds" % m, ["k_kmerize_lds<31>"], lds[:6], m=m, runs=[(1.0, {})]))
        cases.append(_case("m%d_k21" % m, ["k_kmerize_wave<0>"], short21[:6], m=m, k=21, runs=[(1.0, {})]))
        cases.append(_case("m%d_lds_k21" % m, ["k_kmerize_lds<0>", "k_kmer_rows<0>"], long21[:5], m=m, k=21, runs=[(1.0, {}), (1.0, dict(k1_global=True))]))
        cases.append(_case("m%d_parts8" % m, ["k_kmerize_lds<31>"], parts[:1] + lds[:2], m=m, runs=[(0.5, {})]))
        cases.append(_case("m%d_parts8_k21" % m, ["k_kmerize_lds<0>"], [repeat_query(rng, 300, [(0, 299)], 21)] + long21[3:5], m=m, k=21, runs=[(0.5, {})]))
    # ---- what of B the CPU twin must see (planted("k31") / planted("k21")), chosen by name, not by a stride
    TWIN_B[K] = (dedupe + aba(FP31_PAIRS)[:2] + aba(FNV31_PAIRS)[:2] + [wrap_query(FNV31_LAST, K, fnv_fold, (256,)), parts[6], sort_q[len(lds)], many31[2]] +
                 [homopolymer(n, K) for n in (1, 63, 64, 256, 1024)] + short[-2:] + wave64[6:8])
    TWIN_A[K] = lds
    TWIN_B[21] = long21 + short21 + [homopolymer(n, 21) for n in (256, 1024)] + many21[2:3]
    TWIN_A[21] = []
    return cases


TWIN_A, TWIN_B = {}, {}
RUNTIME_KS = (1, 2, 3, 4, 20, 23, 30, 32, 33)


def runtime_js(k):
    last = -(-k // 2) - 1
    return sorted({0, last // 2, last})


RUNTIME_SHAPES = {k: make_shapes(k, runtime_js(k), 100 + k) for k in RUNTIME_KS}
CASES = _build_cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# --------------------------------------------------------------------------------------------- one-call searches on a planted index
def one_call_sequences(seed=11):
    """[(class, sequence)]: one sequence per call.  "read": at most 93 bytes (k_reads_fused, bytes in the arguments), 33 calls of one
    shape each, the alignment rotating; "arg1024": 95 .. 1024 bytes; "arg3072": 1025 .. 3072; "pinned": above 3072 bytes, at most
    4096 positions.  Every longer class holds all 132 placements."""
    rng, out = random.Random(seed), []
    for i, (key, _) in enumerate(SHAPES):
        s, _ = place(rng, [(key, i % 4)], tail=(i * 7) % 50)
        out.append(("read", s))
    for cls, lo, hi in (("arg1024", 95, 1024), ("arg3072", 1025, 3072), ("pinned", 3073, LDS_MAX_POS + K - 1)):
        out += [(cls, s) for s in packed_queries(rng, sorted(PLACEMENTS, key=lambda it: it[1]), hi, lo)]      # (alignment-major: every sequence holds late shapes)
    return out


ONE_CALL = one_call_sequences()
assert len(ONE_CALL) <= 64


class Planted(object):
    """The planted index of at most 64 sequences, from the REFERENCE's rows: column c holds exactly the rows of every k-mer of
    sequence c, column c + 64 the same minus ONE row of one k-mer (a deep shape where the sequence has one, else its first k-mer).
    row_ids / packed: the rows to write (set_rows); expected(seq, thr): (n, u, min_kmers, colours, counts) by the reference over the
    planted matrix itself, so that chance coincidences are accounted for."""

    def __init__(self, seqs, k, h=H, m=M):
        assert len(seqs) <= 64
        self.seqs, self.k, self.h, self.m = seqs, k, h, m
        self.cols = [set() for _ in range(N_COLS)]
        self.dropped = {}
        for c, s in enumerate(seqs):
            r = ref_of(s, k)
            if r.u == 0:
                continue
            rows = r.rows(h, m)
            every = set(x for kr in rows for x in kr)
            self.cols[c] = every
            depth = [first_difference(km)[0] or 0 for km in r.uniq]
            pick = depth.index(max(depth))              # the k-mer whose canonical choice is decided latest
            # (a row that no other k-mer of the sequence shares, where there is one: the k-mer then misses column c + 64)
            others = set(x for t, kr in enumerate(rows) if t != pick for x in kr)
            own = [x for x in rows[pick] if x not in others]
            self.dropped[c] = (pick, own[0] if own else rows[pick][0])
            self.cols[c + 64] = every - {self.dropped[c][1]}
        ids = sorted(set().union(*self.cols))
        self.row_ids = ids
        self.bits = {row: [row in col for col in self.cols] for row in ids}

    def packed(self):
        import numpy as np
        bits = np.array([self.bits[r] for r in self.row_ids], np.uint8).reshape(len(self.row_ids), N_COLS)
        return np.array(self.row_ids, np.uint64), np.packbits(bits, axis=1)

    def expected(self, seq, thr):
        r = ref_of(seq, self.k)
        counts = [0] * N_COLS
        for kr in r.rows(self.h, self.m):
            for c in range(N_COLS):
                if all(x in self.cols[c] for x in kr):
                    counts[c] += 1
        mk = ceil_thr(r.u, thr)
        hit = [c for c in range(N_COLS) if (counts[c] == r.u and r.u > 0 if thr == 1.0 else counts[c] >= mk)]
        return r.n, r.u, mk, hit, [counts[c] for c in hit]


_planted = {}


def planted(name):
    """the planted indexes: "one_call" (ONE_CALL's sequences) and, for the CPU twin, "k<k>": up to 64 sequences of the batch cases
    of that k.  Built once, shared, never changed."""
    if name not in _planted:
        if name == "one_call":
            _planted[name] = Planted([s for _, s in ONE_CALL], K)
        else:
            k = int(name[1:])
            if k in TWIN_B:          # k = 31, 21: every B query by name, and (k = 31) the LDS queries that hold all 132 placements
                seqs = list(dict.fromkeys(TWIN_B[k] + TWIN_A[k]))
            else:
                seqs = []
                for c in CASES:
                    if c["k"] == k and c["m"] == M:
                        seqs += [q for q in c["queries"] if q not in seqs]
            assert len(seqs) <= 64, (name, len(seqs))
            _planted[name] = Planted(seqs, k)
    return _planted[name]
